"""Pairs, query triangles and host-side expectations for the triangle overlap query (tests only).

`Lists.expected` builds a query's answer as the header defines it, from mrt_triangle_overlap over the scene
accessors and nothing else (overlap_cases.Lists with the triangle functions for the box functions).  The
yardsticks are float64 evaluations on the stored float32 corners, the scene side's formed in float32 as
overlap_cases.corners32 does:
  sat23_f64      the 23-axis separating-axis test without slack - exact intersection of the closed shapes, up to
                 float64 rounding - contract (a)'s yardstick;
  distance_f64   the least of the six corner-to-triangle and the nine edge-to-edge distances: the distance
                 between two shapes that do not intersect - with sat23_f64, contract (b)'s yardstick.
"""
import numpy as np

import neighbour_cases as NB
import overlap_cases as C

f32 = np.float32
EPS = C.EPS
G = 64.0  # kTriOverlapG: the measured distance, in eps M, that explains every acceptance (the tests pin 4 G)
PLANE, SPHERE, TRIANGLE, LIGHT = C.PLANE, C.SPHERE, C.TRIANGLE, C.LIGHT
FIELDS, WIDTHS, K_MAX, OFFSETS = C.FIELDS, C.WIDTHS, C.K_MAX, C.OFFSETS
corners32 = C.corners32
cut, rows_of, assert_same = C.cut, C.rows_of, C.assert_same


def record(P0, P1, P2):
    """A, AB, AC in float32 for corners given in float64: A = fl(P0), AB = fl(fl(P1) - A), AC = fl(fl(P2) - A)."""
    A = np.asarray(P0, np.float64).astype(f32)
    return np.concatenate([A, np.asarray(P1, np.float64).astype(f32) - A, np.asarray(P2, np.float64).astype(f32) - A], 1)


def query_corners(q):
    q = np.ascontiguousarray(q, f32).reshape(-1, 9)
    return q[:, :3], q[:, 3:6], q[:, 6:]


# ---- the contract's pairs ------------------------------------------------------------------------------
def contract_pairs(n, seed, offset):
    """(scene triangle, query triangle) pairs at `offset`: every corner offset + centre + U(-1, 1)^3, each
    triangle with its own centre from U(-0.5, 0.5)^3."""
    rng = np.random.default_rng(seed)
    sign = offset * rng.choice([-1.0, 1.0], (n, 1, 3))
    P = sign + rng.uniform(-0.5, 0.5, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3))
    Q = sign + rng.uniform(-0.5, 0.5, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3))
    return record(P[:, 0], P[:, 1], P[:, 2]), Q.reshape(n, 9).astype(f32)


def coplanar_pairs(n, seed):
    """Pairs lying in one axis-aligned plane, exactly: the plane's coordinate is one float32 value for all six
    corners (AB and AC are 0 on that axis, so fl(A + AB) keeps it).  Over the offsets."""
    rng = np.random.default_rng(seed)
    off = rng.choice(OFFSETS, (n, 1, 1)) * rng.choice([-1.0, 1.0], (n, 1, 3))
    P = off + rng.uniform(-0.5, 0.5, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3))
    Q = off + rng.uniform(-0.5, 0.5, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3))
    ax = rng.integers(0, 3, n)
    rows = np.arange(n)
    level = P[rows, 0, ax].astype(f32).astype(np.float64)
    for k in range(3):
        P[rows, k, ax] = level
        Q[rows, k, ax] = level
    return record(P[:, 0], P[:, 1], P[:, 2]), Q.reshape(n, 9).astype(f32)


def shared_pairs(n, seed, corners):
    """Pairs sharing `corners` (1 or 2) stored corners bit for bit - a mesh against itself: the query's first
    corners are the scene triangle's P0 (and P1 = fl(A + AB)), in a random rotation of both triangles."""
    tri, q = contract_pairs(n, seed, 0.0)
    rng = np.random.default_rng(seed + 1)
    off = (rng.choice(OFFSETS, (n, 1)) * rng.choice([-1.0, 1.0], (n, 3))).astype(f32)
    P = [p + off for p in corners32(tri)]
    tri = np.concatenate([P[0], P[1] - P[0], P[2] - P[0]], 1).astype(f32)
    P = corners32(tri)
    Q = q.reshape(n, 3, 3) + off[:, None, :]
    Q[:, 0] = P[0]
    if corners == 2:
        Q[:, 1] = P[1]
    roll = rng.integers(0, 3, n)
    Q = np.stack([Q[np.arange(n), (roll + k) % 3] for k in range(3)], 1)
    return tri, Q.reshape(n, 9).astype(f32)


def segment_pairs(n, seed):
    """Query segments (two corners equal, in every arrangement) against proper triangles, over the offsets; a
    third of the segments have an end on the triangle (a float32 point of it)."""
    rng = np.random.default_rng(seed)
    parts = [contract_pairs(n // 4, seed + 10 + i, off) for i, off in enumerate(OFFSETS)]
    tri, q = np.concatenate([p for p, _ in parts]), np.concatenate([x for _, x in parts])
    Q = q.reshape(-1, 3, 3)
    rows = rng.random(len(tri)) < 1 / 3
    t = tri[rows].astype(np.float64)
    w = rng.random((int(rows.sum()), 2))
    w[w.sum(1) > 1] = 1 - w[w.sum(1) > 1]
    Q[rows, 0] = (t[:, :3] + w[:, :1] * t[:, 3:6] + w[:, 1:] * t[:, 6:]).astype(f32)
    same = rng.integers(0, 3, len(Q))  # which corner repeats its neighbour
    idx = np.arange(len(Q))
    Q[idx, same] = Q[idx, (same + 1) % 3]
    return tri, Q.reshape(-1, 9).astype(f32)


def point_pairs(n, seed):
    """Query points (three equal corners) against proper triangles, over the offsets: points of the triangle as
    float32 rounds them, moved along the normal by 0 or by 1e-8 .. 1 sizes, a tenth moved sideways too."""
    rng = np.random.default_rng(seed)
    parts = [contract_pairs(n // 4, seed + 10 + i, off) for i, off in enumerate(OFFSETS)]
    tri = np.concatenate([p for p, _ in parts])
    t = tri.astype(np.float64)
    m = len(tri)
    w = rng.random((m, 2))
    w[w.sum(1) > 1] = 1 - w[w.sum(1) > 1]
    w[rng.random(m) < 0.1] = (0.0, 0.0)  # the corner A
    nr = np.cross(t[:, 3:6], t[:, 6:])
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    dist = np.where(rng.random((m, 1)) < 0.3, 0.0, 10.0 ** rng.uniform(-8, 0, (m, 1))) * rng.choice([-1.0, 1.0], (m, 1))
    side = rng.normal(size=(m, 3)) * (rng.random((m, 1)) < 0.1)
    p = (t[:, :3] + w[:, :1] * t[:, 3:6] + w[:, 1:] * t[:, 6:] + nr * dist + side).astype(f32)
    return tri, np.concatenate([p, p, p], 1)


def degenerate_pairs(n, seed):
    """Both shapes degenerate (contract (a) only): scene segments and points against query segments and
    points, half of the queries holding one of the scene shape's stored corners bit for bit."""
    tri, q = contract_pairs(n, seed, 0.0)
    rng = np.random.default_rng(seed + 1)
    off = (rng.choice(OFFSETS, (n, 1)) * rng.choice([-1.0, 1.0], (n, 3))).astype(f32)
    tri[:, :3] += off
    tri[:, 6:] = np.where(rng.random((n, 1)) < 0.5, tri[:, 3:6], 0.0)  # AC = AB or 0: a segment
    both = rng.random(n) < 0.3
    tri[both, 3:] = 0.0  # a point
    P = corners32(tri)
    Q = q.reshape(n, 3, 3) + off[:, None, :]
    Q[:, 2] = Q[:, 1]
    pt = rng.random(n) < 0.4
    Q[pt, 1] = Q[pt, 0]
    Q[pt, 2] = Q[pt, 0]
    share = rng.random(n) < 0.5
    Q[share, 0] = np.where(rng.random((int(share.sum()), 1)) < 0.5, P[0][share], P[1][share])
    Q[pt, 1] = Q[pt, 0]
    Q[pt, 2] = Q[pt, 0]
    return tri, Q.reshape(n, 9).astype(f32)


def plane_pairs(n, seed):
    """(plane, triangle) pairs over the offsets: unit normals (a third along an axis), triangles of 1e-3 .. 0.5
    sizes about points at 0 or 1e-4 .. 100 sizes from the plane."""
    rng = np.random.default_rng(seed)
    off = rng.choice(OFFSETS, (n, 1))
    size = 10.0 ** rng.uniform(-3, np.log10(2.0), (n, 1))
    nr = rng.normal(size=(n, 3))
    ax = rng.random(n) < 1 / 3
    nr[ax] = np.eye(3)[rng.integers(0, 3, int(ax.sum()))]
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    nr = nr.astype(f32).astype(np.float64)
    pt = off * rng.choice([-1.0, 1.0], (n, 3)) + rng.uniform(-1, 1, (n, 3)) * size
    t = rng.normal(size=(n, 3))
    t -= (t * nr).sum(1, keepdims=True) * nr
    dist = np.where(rng.random((n, 1)) < 0.05, 0.0, 10.0 ** rng.uniform(-4, 2, (n, 1))) * rng.choice([-1.0, 1.0], (n, 1))
    c = pt + t * size + nr * dist * size
    h = size * 10.0 ** rng.uniform(-3, -0.3, (n, 1))
    Q = c[:, None, :] + rng.uniform(-1, 1, (n, 3, 3)) * h[:, None, :]
    return np.concatenate([nr, pt], 1).astype(f32), Q.reshape(n, 9).astype(f32)


def sphere_pairs(n, seed):
    """(sphere, triangle) pairs over the offsets: radii 1e-3 .. 2, triangles about points near the surface."""
    rng = np.random.default_rng(seed)
    off = rng.choice(OFFSETS, (n, 1))
    rad = 10.0 ** rng.uniform(-3, np.log10(2.0), (n, 1))
    ce = off * rng.choice([-1.0, 1.0], (n, 3)) + rng.uniform(-1, 1, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = np.where(rng.random((n, 1)) < 0.05, 0.0, 10.0 ** rng.uniform(-4, 1.5, (n, 1))) * rng.choice([-1.0, 1.0], (n, 1))
    c = ce + d * rad * (1.0 + dist)
    h = rad * 10.0 ** rng.uniform(-3, -0.3, (n, 1))
    Q = c[:, None, :] + rng.uniform(-1, 1, (n, 3, 3)) * h[:, None, :]
    return np.concatenate([ce, rad * rad], 1).astype(f32), Q.reshape(n, 9).astype(f32)


def scale_of(kind, prims, q):
    """M: the largest |coordinate| of the primitive's points and the query's corners (a sphere: its radius too)."""
    prims = np.ascontiguousarray(prims, f32)
    m = np.abs(np.asarray(q, np.float64).reshape(len(prims), 9)).max(1)
    if kind in (TRIANGLE, LIGHT):
        for P in corners32(prims):
            m = np.maximum(m, np.abs(P.astype(np.float64)).max(1))
    elif kind == PLANE:
        m = np.maximum(m, np.abs(prims[:, 3:6].astype(np.float64)).max(1))
    else:
        m = np.maximum(m, np.maximum(np.abs(prims[:, :3].astype(np.float64)).max(1), np.sqrt(prims[:, 3].astype(np.float64))))
    return m


# ---- the float64 yardsticks ----------------------------------------------------------------------------
def _shapes64(tri, q):
    """The six corners in float64, moved by the scene triangle's first corner (exact in float64 here)."""
    P = [p.astype(np.float64) for p in corners32(tri)]
    Q = [x.astype(np.float64) for x in query_corners(q)]
    o = P[0].copy()
    return [p - o for p in P], [x - o for x in Q]


def _cross3(a, b):
    """The cross product of two (3, n) arrays."""
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def sat23_f64(tri, q):
    """True: none of the 23 axes (and none of the three coordinate axes) separates the two closed triangles.
    Components first ((3, n) arrays), and each family of axes only on the pairs the earlier ones left."""
    n = len(tri)
    P, Q = _shapes64(tri, q)
    P, Q = [np.ascontiguousarray(p.T) for p in P], [np.ascontiguousarray(x.T) for x in Q]
    ok = np.ones(n, bool)

    def run(families):
        live = np.nonzero(ok)[0]
        if not len(live):
            return
        p, x = [c[:, live] for c in P], [c[:, live] for c in Q]
        e = [p[1] - p[0], p[2] - p[1], p[0] - p[2]]
        f = [x[1] - x[0], x[2] - x[1], x[0] - x[2]]
        nP, nQ = _cross3(e[0], e[1]), _cross3(f[0], f[1])
        keep = np.ones(len(live), bool)
        for a in families(e, f, nP, nQ):
            u = [a[0] * c[0] + a[1] * c[1] + a[2] * c[2] for c in p]
            v = [a[0] * c[0] + a[1] * c[1] + a[2] * c[2] for c in x]
            umin, umax = np.minimum(np.minimum(u[0], u[1]), u[2]), np.maximum(np.maximum(u[0], u[1]), u[2])
            vmin, vmax = np.minimum(np.minimum(v[0], v[1]), v[2]), np.maximum(np.maximum(v[0], v[1]), v[2])
            keep &= ~((umin > vmax) | (vmin > umax))
        ok[live[~keep]] = False

    run(lambda e, f, nP, nQ: [np.eye(3)[:, k:k + 1] for k in range(3)] + [nP, nQ])  # the hulls, the normals
    run(lambda e, f, nP, nQ: [_cross3(a, b) for a in e for b in f])
    run(lambda e, f, nP, nQ: [_cross3(nP, a) for a in e] + [_cross3(nQ, b) for b in f]
        + [_cross3(nP, b) for b in f] + [_cross3(nQ, a) for a in e])
    return ok


def _dot(a, b):
    return (a * b).sum(1)


def point_segment_f64(p, a, b):
    d = b - a
    dd = _dot(d, d)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(dd > 0, np.clip(_dot(p - a, d) / np.where(dd > 0, dd, 1.0), 0.0, 1.0), 0.0)
    return np.linalg.norm(p - (a + d * s[:, None]), axis=1)


def point_triangle_f64(p, a, b, c):
    """The distance from p to the closed triangle a, b, c (any of them degenerate)."""
    d = np.minimum(np.minimum(point_segment_f64(p, a, b), point_segment_f64(p, b, c)), point_segment_f64(p, c, a))
    ab, ac, ap = b - a, c - a, p - a
    n = np.cross(ab, ac)
    nn = _dot(n, n)
    safe = np.where(nn > 0, nn, 1.0)
    u = _dot(np.cross(ap, ac), n) / safe
    v = _dot(np.cross(ab, ap), n) / safe
    inside = (nn > 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
    face = np.abs(_dot(ap, n)) / np.sqrt(safe)
    return np.where(inside, np.minimum(d, face), d)


def segment_segment_f64(p1, q1, p2, q2):
    """Ericson's closest points of two segments (Real-Time Collision Detection 5.1.9), degenerate ones included.
    Never below the true distance; for near-parallel segments the corner-to-triangle terms hold the minimum."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f, c, b = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
    den = a * e - b * b
    sa, se = np.where(a > 0, a, 1.0), np.where(e > 0, e, 1.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.where((den > 0) & (a > 0), np.clip((b * f - c * e) / np.where(den > 0, den, 1.0), 0.0, 1.0), 0.0)
        t = np.where(e > 0, (b * s + f) / se, 0.0)
        s = np.where(t < 0, np.where(a > 0, np.clip(-c / sa, 0.0, 1.0), 0.0),
                     np.where(t > 1, np.where(a > 0, np.clip((b - c) / sa, 0.0, 1.0), 0.0), s))
    t = np.clip(t, 0.0, 1.0)
    return np.linalg.norm((p1 + d1 * s[:, None]) - (p2 + d2 * t[:, None]), axis=1)


def distance_f64(tri, q):
    """The least of the six corner-to-triangle and the nine edge-to-edge distances."""
    P, Q = _shapes64(tri, q)
    d = np.full(len(tri), np.inf)
    for p in P:
        d = np.minimum(d, point_triangle_f64(p, *Q))
    for x in Q:
        d = np.minimum(d, point_triangle_f64(x, *P))
    for i in range(3):
        for j in range(3):
            d = np.minimum(d, segment_segment_f64(P[i], P[(i + 1) % 3], Q[j], Q[(j + 1) % 3]))
    return d


def triangle_f64(tri, q, grow=0.0):
    """(b)'s yardstick: the float64 test accepts, or the two shapes are within `grow` (a number or one per pair)."""
    ok = sat23_f64(tri, q)
    g = np.broadcast_to(np.asarray(grow, np.float64), (len(tri),))
    rest = ~ok & (g > 0)
    if rest.any():
        ok[rest] = distance_f64(tri[rest], q[rest]) <= g[rest]
    return ok


def plane_f64(prims, q, grow=0.0):
    """The plane against the closed triangle: the corners are not all strictly on one side, or the nearest is
    within `grow`."""
    p = prims.astype(np.float64)
    s = np.stack([_dot(p[:, :3], x.astype(np.float64) - p[:, 3:6]) for x in query_corners(q)])
    g = np.broadcast_to(np.asarray(grow, np.float64), (len(p),)) * np.linalg.norm(p[:, :3], axis=1)
    return (s.min(0) <= g) & (s.max(0) >= -g)


def sphere_f64(prims, q, grow=0.0):
    """The sphere's surface against the closed triangle: the nearest point inside or on, the farthest corner
    outside or on, each within `grow`."""
    p = prims.astype(np.float64)
    Q = [x.astype(np.float64) for x in query_corners(q)]
    ce, R = p[:, :3], np.sqrt(p[:, 3])
    g = np.broadcast_to(np.asarray(grow, np.float64), (len(p),))
    near = point_triangle_f64(ce, *Q)
    far = np.max([np.linalg.norm(x - ce, axis=1) for x in Q], axis=0)
    return (near <= R + g) & (far >= R - g)


F64 = {PLANE: plane_f64, SPHERE: sphere_f64, TRIANGLE: triangle_f64, LIGHT: triangle_f64}


def hulls_overlap(tri, q):
    """The cull's premise in float32: the hull of A, fl(A + AB), fl(A + AC) against the query's, closed compares."""
    P, Q = corners32(tri), query_corners(q)
    lo, hi = np.minimum(np.minimum(P[0], P[1]), P[2]), np.maximum(np.maximum(P[0], P[1]), P[2])
    qlo, qhi = np.minimum(np.minimum(Q[0], Q[1]), Q[2]), np.maximum(np.maximum(Q[0], Q[1]), Q[2])
    assert lo.dtype == f32 and qlo.dtype == f32
    return ~((lo > qhi) | (hi < qlo)).any(1)


def hull_of(q):
    """(n, 6): the query triangles' hulls, mn xyz and mx xyz, in float32."""
    Q = query_corners(q)
    return np.concatenate([np.minimum(np.minimum(Q[0], Q[1]), Q[2]), np.maximum(np.maximum(Q[0], Q[1]), Q[2])], 1)


# ---- query triangles for a scene ---------------------------------------------------------------------------
def scene_queries(geom, n, seed, extent):
    """n query triangles (n a multiple of 6, at least 12) about the triangles `geom` (count, 3, 3: A, AB, AC):
    points of the surface and corners (three equal corners), segments between surface points, triangles from
    1e-3 * extent to the whole scene's size about surface points, the scene's own triangles (its stored corners
    bit for bit: a mesh against itself), and triangles thrown into the scene's box."""
    rng = np.random.default_rng(seed)
    per = n // 6
    flat = geom.reshape(-1, 9)
    c = NB.corners_of(geom)
    lo, hi = c.min(0).astype(np.float64), c.max(0).astype(np.float64)
    on = NB.surface_points(flat, per // 2, rng, 0.0).astype(f32)
    cor = NB.corner_points(flat, per - per // 2, rng).astype(f32)
    pts = np.concatenate([on, cor])
    parts = [np.concatenate([pts, pts, pts], 1)]
    a = NB.surface_points(flat, per, rng, 0.0)
    b = a + rng.normal(size=(per, 3)) * extent * 10.0 ** rng.uniform(-3, 0, (per, 1))
    seg = np.stack([a, b, b], 1)
    roll = rng.integers(0, 3, per)
    parts.append(np.stack([seg[np.arange(per), (roll + k) % 3] for k in range(3)], 1).reshape(per, 9).astype(f32))
    for _ in range(2):
        ce = NB.surface_points(flat, per, rng, 0.01 * extent)
        h = extent * 10.0 ** rng.uniform(-3, 0, (per, 1, 1)) * 0.5
        parts.append((ce[:, None, :] + rng.uniform(-1, 1, (per, 3, 3)) * h).reshape(per, 9).astype(f32))
    own = geom[rng.integers(0, len(geom), per)].reshape(per, 9)
    parts.append(np.concatenate(corners32(own), 1))
    rest = per - 1
    parts.append(rng.uniform(lo, hi, (rest, 3, 3)).reshape(rest, 9).astype(f32))
    whole = np.concatenate([lo - 1, (hi[0] + 1, lo[1] - 1, hi[2] + 1), (lo[0] - 1, hi[1] + 1, hi[2] + 1)])[None, :]
    tris = np.concatenate(parts + [whole.astype(f32)]).astype(f32)
    assert tris.shape == (n, 9)
    return tris


# ---- a query's expected answers ------------------------------------------------------------------------
class Lists(C.Lists):
    """overlap_cases.Lists with mrt_triangle_overlap for mrt_box_overlap: the candidates of cfg's scene as
    columns in (kind, input index) order, and the expected lists."""

    def accepted(self, tris, chunk=256):
        """mrt_triangle_overlap of every (candidate, query triangle) pair: (n, candidates) bool."""
        import mobileraytracer_amd as m
        tris = np.ascontiguousarray(tris, f32).reshape(-1, 9)
        out = np.zeros((len(tris), len(self.kind)), bool)
        for k, rec in self.rec.items():
            T, c0 = len(rec), self.first[k]
            for a in range(0, len(tris), chunk):
                tx = tris[a:a + chunk]
                out[a:a + chunk, c0:c0 + T] = m.triangle_overlap(k, np.tile(rec, (len(tx), 1)),
                                                                 np.repeat(tx, T, 0)).reshape(len(tx), T) != 0
        return out & self.valid[None, :]
