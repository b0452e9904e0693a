"""Pairs, boxes and host-side expectations for the overlap query (tests only).

`Lists.expected` builds a query's answer as the header defines it, from mrt_box_overlap over the scene
accessors and nothing else: the function's verdict on every (candidate, box) pair, count = the accepted
candidates, the list their first K in (kind, input index) order, then the padding.  Nothing of the walk is
restated here.  `sat_f64` is the contract's yardstick: the 13-axis separating-axis test in float64, without
slack, on the stored float32 corners A, fl(A + AB), fl(A + AC).
"""
import numpy as np

import nearest_cases as N
import neighbour_cases as NB

f32 = np.float32
EPS = 2.0 ** -24
G = 64.0  # kOverlapG: the measured growth, in eps M, that explains every acceptance (the tests pin 4 G)
PLANE, SPHERE, TRIANGLE, LIGHT = N.PLANE, N.SPHERE, N.TRIANGLE, N.LIGHT
FIELDS = ("any", "count", "kind", "index")  # every field but `tests`
WIDTHS = {"any": 0, "count": 0, "kind": 1, "index": 1, "tests": 0}  # 0: one per box
K_MAX = 16
OFFSETS = (0.0, 100.0, 1024.0, 4096.0)


# ---- the contract's pairs ------------------------------------------------------------------------------
def corners32(tri):
    """P0, P1, P2 as aabbOf forms them: A, fl(A + AB), fl(A + AC) in float32."""
    tri = np.ascontiguousarray(tri, f32)
    A = tri[:, :3]
    return A, A + tri[:, 3:6], A + tri[:, 6:]


def triangle_pairs(n, seed, offset):
    """(triangle, box) pairs at `offset`: sizes 1e-3 .. 2 (log uniform), a tenth slivers, a twentieth
    degenerate (AC = 0, or AB = AC = 0); boxes of 0.01 .. 1 sizes per axis (a twentieth of zero extent), half
    of them with a corner, the others with their centre, at a random distance (0, or 1e-7 .. 10 sizes) along
    the triangle's normal from a point of the triangle - near its plane, so that a good share overlaps."""
    rng = np.random.default_rng(seed)
    size = 10.0 ** rng.uniform(-3, np.log10(2.0), (n, 1))
    A = offset * rng.choice([-1.0, 1.0], (n, 3)) + rng.uniform(-1, 1, (n, 3)) * size
    AB = rng.normal(size=(n, 3))
    AB *= size / np.linalg.norm(AB, axis=1, keepdims=True)
    AC = rng.normal(size=(n, 3))
    AC *= size * rng.uniform(0.25, 1.0, (n, 1)) / np.linalg.norm(AC, axis=1, keepdims=True)
    kind = rng.random(n)
    sl = kind < 0.1
    AC[sl] = rng.uniform(-2, 2, (int(sl.sum()), 1)) * AB[sl] + 1e-5 * size[sl] * rng.normal(size=(int(sl.sum()), 3))
    dg = (kind >= 0.1) & (kind < 0.15)
    both = dg & (rng.random(n) < 0.5)
    AC[dg] = 0.0
    AB[both] = 0.0
    w = rng.random((n, 2))
    w[w.sum(1) > 1] = 1 - w[w.sum(1) > 1]
    on = A + w[:, :1] * AB + w[:, 1:] * AC
    nrm = np.cross(AB, AC)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    rnd = rng.normal(size=(n, 3))
    nrm = np.where(ln > 1e-12 * size * size, nrm / np.where(ln > 0, ln, 1), rnd / np.linalg.norm(rnd, axis=1, keepdims=True))
    dist = np.where(rng.random((n, 1)) < 0.1, 0.0, 10.0 ** rng.uniform(-7, 1.0, (n, 1))) * rng.choice([-1.0, 1.0], (n, 1))
    h = size * 10.0 ** rng.uniform(-2, 0, (n, 3)) * 0.5
    h[rng.random(n) < 0.05] = 0.0
    corner = rng.choice([-1.0, 1.0], (n, 3)) * (rng.random((n, 1)) < 0.5)  # (0, 0, 0: the centre)
    slide = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 0.9, (n, 1)) * (rng.random((n, 1)) < 0.9)  # off the triangle
    c = on + nrm * dist * size + corner * h + slide * size
    box = np.concatenate([c - h, c + h], 1).astype(f32)
    box[:, 3:] = np.maximum(box[:, :3], box[:, 3:])
    return np.concatenate([A, AB, AC], 1).astype(f32), box


def plane_pairs(n, seed):
    """(plane, box) pairs over the offsets: unit normals (a third along an axis), boxes near the plane."""
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
    h = size * 10.0 ** rng.uniform(-3, -0.3, (n, 3)) * 0.5
    h[rng.random(n) < 0.05] = 0.0
    c = pt + t * size + nr * dist * size
    box = np.concatenate([c - h, c + h], 1).astype(f32)
    box[:, 3:] = np.maximum(box[:, :3], box[:, 3:])
    return np.concatenate([nr, pt], 1).astype(f32), box


def sphere_pairs(n, seed):
    """(sphere, box) pairs over the offsets: radii 1e-3 .. 2, boxes about points near the surface."""
    rng = np.random.default_rng(seed)
    off = rng.choice(OFFSETS, (n, 1))
    rad = 10.0 ** rng.uniform(-3, np.log10(2.0), (n, 1))
    ce = off * rng.choice([-1.0, 1.0], (n, 3)) + rng.uniform(-1, 1, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = np.where(rng.random((n, 1)) < 0.05, 0.0, 10.0 ** rng.uniform(-4, 1.5, (n, 1))) * rng.choice([-1.0, 1.0], (n, 1))
    h = rad * 10.0 ** rng.uniform(-3, -0.3, (n, 3)) * 0.5
    h[rng.random(n) < 0.05] = 0.0
    c = ce + d * rad * (1.0 + dist)
    box = np.concatenate([c - h, c + h], 1).astype(f32)
    box[:, 3:] = np.maximum(box[:, :3], box[:, 3:])
    return np.concatenate([ce, rad * rad], 1).astype(f32), box


def scale_of(kind, prims, box):
    """M: the largest |coordinate| of the primitive's points and the bounds (a sphere: its radius too)."""
    prims = np.ascontiguousarray(prims, f32)
    m = np.abs(box.astype(np.float64)).max(1)
    if kind in (TRIANGLE, LIGHT):
        for P in corners32(prims):
            m = np.maximum(m, np.abs(P.astype(np.float64)).max(1))
    elif kind == PLANE:
        m = np.maximum(m, np.abs(prims[:, 3:6].astype(np.float64)).max(1))
    else:
        m = np.maximum(m, np.maximum(np.abs(prims[:, :3].astype(np.float64)).max(1), np.sqrt(prims[:, 3].astype(np.float64))))
    return m


def sat_f64(tri, box, grow=0.0):
    """The 13-axis test in float64 without slack on the stored float32 corners; the box grown by `grow`
    (a number or one per pair) on every side.  True: no axis separates the triangle from the closed box."""
    P = [p.astype(np.float64) for p in corners32(tri)]
    b = box.astype(np.float64)
    g = np.broadcast_to(np.asarray(grow, np.float64), (len(b),))[:, None]
    mn, mx = b[:, :3] - g, b[:, 3:] + g
    c, h = (mn + mx) * 0.5, (mx - mn) * 0.5
    v = [p - c for p in P]
    lo, hi = np.minimum(np.minimum(v[0], v[1]), v[2]), np.maximum(np.maximum(v[0], v[1]), v[2])
    ok = ~((lo > h) | (hi < -h)).any(1)
    e = [v[1] - v[0], v[2] - v[1], v[0] - v[2]]

    def axis(a):
        p = np.stack([(a * x).sum(1) for x in v])
        r = (h * np.abs(a)).sum(1)
        return ~((p.min(0) > r) | (p.max(0) < -r))

    for i in range(3):
        u = np.zeros(3)
        u[i] = 1.0
        for ej in e:
            ok &= axis(np.cross(np.broadcast_to(u, ej.shape), ej))
    ok &= axis(np.cross(e[0], e[1]))
    return ok


def plane_f64(prims, box, grow=0.0):
    p, b = prims.astype(np.float64), box.astype(np.float64)
    g = np.broadcast_to(np.asarray(grow, np.float64), (len(b),))[:, None]
    mn, mx = b[:, :3] - g, b[:, 3:] + g
    c, h = (mn + mx) * 0.5, (mx - mn) * 0.5
    return np.abs((p[:, :3] * (c - p[:, 3:6])).sum(1)) <= (h * np.abs(p[:, :3])).sum(1)


def sphere_f64(prims, box, grow=0.0):
    """The sphere's surface against the closed box: nearest point inside or on, farthest corner outside or on."""
    p, b = prims.astype(np.float64), box.astype(np.float64)
    g = np.broadcast_to(np.asarray(grow, np.float64), (len(b),))[:, None]
    mn, mx = b[:, :3] - g, b[:, 3:] + g
    ce = p[:, :3]
    near = np.maximum(np.maximum(mn - ce, ce - mx), 0.0)
    far = np.maximum(np.abs(ce - mn), np.abs(mx - ce))
    return ((near * near).sum(1) <= p[:, 3]) & ((far * far).sum(1) >= p[:, 3])


F64 = {PLANE: plane_f64, SPHERE: sphere_f64, TRIANGLE: sat_f64, LIGHT: sat_f64}


def hull_overlaps(tri, box):
    """The cull's premise in float32: the hull of A, fl(A + AB), fl(A + AC) against the box, closed compares."""
    P = corners32(tri)
    lo, hi = np.minimum(np.minimum(P[0], P[1]), P[2]), np.maximum(np.maximum(P[0], P[1]), P[2])
    assert lo.dtype == f32
    return ~((lo > box[:, 3:]) | (hi < box[:, :3])).any(1)


# ---- boxes for a scene -----------------------------------------------------------------------------------
def scene_boxes(geom, n, seed, extent):
    """n boxes (n a multiple of 6, at least 12) about the triangles `geom` (count, 3, 3: A, AB, AC): zero-extent
    boxes on surface points and on corners, cubes from 1e-3 * extent to the whole scene box, thin slabs, and one
    box per axis that only touches the scene box's face."""
    rng = np.random.default_rng(seed)
    per = n // 6
    c = NB.corners_of(geom)
    lo, hi = c.min(0).astype(f32), c.max(0).astype(f32)
    flat = geom.reshape(-1, 9)
    on = NB.surface_points(flat, per, rng, 0.0).astype(f32)
    cor = NB.corner_points(flat, per, rng).astype(f32)
    parts = [np.concatenate([on, on], 1), np.concatenate([cor, cor], 1)]
    for k in range(2):
        ce = NB.surface_points(flat, per, rng, 0.01 * extent)
        h = extent * 10.0 ** rng.uniform(-3, 0, (per, 1)) * 0.5
        parts.append(np.concatenate([ce - h, ce + h], 1).astype(f32))
    ce = NB.surface_points(flat, per, rng, 0.01 * extent)
    h = extent * 10.0 ** rng.uniform(-2, 0, (per, 3)) * 0.5
    h[np.arange(per), rng.integers(0, 3, per)] = 0.0  # slabs: no extent on one axis
    parts.append(np.concatenate([ce - h, ce + h], 1).astype(f32))
    rest = per - 4
    ce = rng.uniform(lo, hi, (rest, 3))
    h = extent * 10.0 ** rng.uniform(-1.5, 0, (rest, 3)) * 0.5
    parts.append(np.concatenate([ce - h, ce + h], 1).astype(f32))
    whole = np.concatenate([lo, hi])[None, :]
    touch = []
    for a in range(3):  # mx.a == the scene box's mn.a: closed boxes touch
        b = np.concatenate([lo - 1, hi + 1]).astype(f32)
        b[3 + a] = lo[a]
        touch.append(b)
    boxes = np.concatenate(parts + [whole, np.array(touch, f32)]).astype(f32)
    boxes[:, 3:] = np.maximum(boxes[:, :3], boxes[:, 3:])
    assert len(boxes) == n
    return boxes


# ---- a query's expected answers ------------------------------------------------------------------------
class Lists:
    """The candidates of cfg's scene as columns in (kind, input index) order, and the expected lists."""

    def __init__(self, cfg, lights_only=False):
        nb = NB.Lists(cfg, lights_only)
        self.rec, self.kind, self.index, self.valid, self.first = nb.rec, nb.kind, nb.index, nb.valid, nb.first

    def accepted(self, boxes, chunk=256):
        """mrt_box_overlap of every (candidate, box) pair: (n, candidates) bool."""
        import mobileraytracer_amd as m
        boxes = np.ascontiguousarray(boxes, f32)
        out = np.zeros((len(boxes), len(self.kind)), bool)
        for k, rec in self.rec.items():
            T, c0 = len(rec), self.first[k]
            for a in range(0, len(boxes), chunk):
                bx = boxes[a:a + chunk]
                out[a:a + chunk, c0:c0 + T] = m.box_overlap(k, np.tile(rec, (len(bx), 1)),
                                                            np.repeat(bx, T, 0)).reshape(len(bx), T) != 0
        return out & self.valid[None, :]

    def expected(self, boxes, k, ok=None):
        """any, count, kind, index as the header defines them (ok: accepted(boxes), if at hand)."""
        ok = self.accepted(boxes) if ok is None else ok
        n, C = ok.shape
        count = ok.sum(1).astype(np.int32)
        # the columns are in (kind, input index) order already: a stable sort on "not accepted" lists them
        order = np.argsort(~ok, axis=1, kind="stable")
        top = np.zeros((n, k), np.int64)
        w = min(k, C)
        top[:, :w] = order[:, :w]
        held = np.arange(k)[None, :] < count[:, None]
        return {"any": (count > 0).astype(np.int32), "count": count,
                "kind": np.where(held, self.kind[top], 0).astype(np.int32),
                "index": np.where(held, self.index[top], -1).astype(np.int32)}


def cut(want, k):
    """The answer for a smaller K from the one for a larger: any and count, and the first k entries."""
    return {f: (x if WIDTHS[f] == 0 else x[:, :k]) for f, x in want.items()}


def rows_of(want, rows):
    return {f: x[rows] for f, x in want.items()}


def assert_same(got, want, what="", fields=FIELDS):
    """Every comparison is exact on ints."""
    for f in fields:
        if f not in want or f not in got:
            continue
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape and g.dtype == np.int32, (what, f, g.shape, w.shape, g.dtype)
        bad = (g != w).reshape(len(g), -1).any(1)
        assert not bad.any(), "%s field %s differs in %d of %d boxes, first %d: got %s want %s" % (
            what, f, bad.sum(), len(g), np.argmax(bad), g[np.argmax(bad)], w[np.argmax(bad)])
