"""Cases and host-side expectations for the nearest-point query (tests only).

The (primitive, point) pairs the CPU test checks mrt_point_distance on - exact, degenerate, sliver and
random ones - are the pairs the GPU test sends through the device functions, and `expected` builds a
query's answers from mrt_point_distance over the scene accessors with the documented total order
(d2, kind, input index): no formula of the distance functions is restated here.
"""
import numpy as np

f32 = np.float32
EPS = 2.0 ** -24
K_KERNEL = 32.0  # kNearestK: the k of the walk's cull
PLANE, SPHERE, TRIANGLE, LIGHT = 1, 2, 3, 4
FIELDS = ("kind", "index", "dist2", "point", "bary")  # every field but `tests`


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


# ---- exact cases -------------------------------------------------------------------------------------
RIGHT = (0, 0, 0, 4, 0, 0, 0, 4, 0)  # A, AB, AC


def exact_triangle():
    """The right triangle and one point in each Voronoi region (power-of-two coordinates): prims, points,
    d2, nearest, bary - all derived by hand."""
    rows = [  # point, d2, nearest, (u, v)
        ((-1, -2, 0), 5, (0, 0, 0), (0, 0)),            # A
        ((6, -1, 2), 9, (4, 0, 0), (1, 0)),             # B
        ((2, -1, 0), 1, (2, 0, 0), (0.5, 0)),           # AB
        ((-1, 8, 0), 17, (0, 4, 0), (0, 1)),            # C
        ((-2, 1, 1), 5, (0, 1, 0), (0, 0.25)),          # AC
        ((4, 4, 0), 8, (2, 2, 0), (0.5, 0.5)),          # BC
        ((1, 0.5, -2), 4, (1, 0.5, 0), (0.25, 0.125)),  # face
    ]
    pts = np.array([r[0] for r in rows], f32)
    return (np.tile(np.array(RIGHT, f32), (len(rows), 1)), pts, np.array([r[1] for r in rows], f32),
            np.array([r[2] for r in rows], f32), np.array([r[3] for r in rows], f32))


def exact_plane():
    prims = np.array([(0, 0, 1, 5, -3, 2), (0, 0, 1, 5, -3, 2), (0, -1, 0, 1, 1, 1), (1, 0, 0, 0, 0, 0)], f32)
    pts = np.array([(3, 4, 4), (3, 4, -2), (2, 4, 8), (0, 7, 7)], f32)
    return (prims, pts, np.array([4, 16, 9, 0], f32), np.array([(3, 4, 2), (3, 4, 2), (2, 1, 8), (0, 7, 7)], f32),
            np.zeros((4, 2), f32))


def exact_sphere():
    prims = np.array([(1, 1, 1, 4)] * 4 + [(0, 0, 0, 0.25)], f32)
    pts = np.array([(1, 1, 1), (1, 5, 1), (2, 1, 1), (1, 1, -1), (0, 0, 0)], f32)
    return (prims, pts, np.array([4, 4, 1, 0, 0.25], f32),
            np.array([(3, 1, 1), (1, 3, 1), (3, 1, 1), (1, 1, -1), (0.5, 0, 0)], f32), np.zeros((5, 2), f32))


def degenerate_triangles(seed=5, per=64):
    """Zero AB, AC == AB, AC == -AB / 2 and corners at 2^40, each with `per` points on, near and far."""
    rng = np.random.default_rng(seed)
    big = 2.0 ** 40
    shapes = [
        ((1, 2, 3), (0, 0, 0), (0.5, 0.25, -1)),
        ((1, 2, 3), (0, 0, 0), (0, 0, 0)),
        ((-1, 0.5, 2), (2, 1, -0.5), (2, 1, -0.5)),
        ((-1, 0.5, 2), (2, 1, -0.5), (-1, -0.5, 0.25)),
        ((big, big, big), (2.0 ** 18, 0, 0), (0, 2.0 ** 18, 2.0 ** 18)),
        ((big, -big, 0), (-2 * big, 2 * big, big), (big, big, -big)),
        ((0, 0, 0), (big, big, big), (big, big, big)),
    ]
    prims, pts = [], []
    for A, AB, AC in shapes:
        A, AB, AC = (np.array(x, np.float64) for x in (A, AB, AC))
        scale = max(np.abs(AB).max(), np.abs(AC).max(), 1.0)
        on = A + rng.random((per, 1)) * AB + rng.random((per, 1)) * 0.5 * AC
        off = rng.normal(size=(per, 3)) * scale * rng.choice([0.0, 1e-6, 1e-3, 1.0, 100.0], (per, 1))
        pts.append(on + off)
        prims.append(np.tile(np.concatenate([A, AB, AC]), (per, 1)))
    return np.concatenate(prims).astype(f32), np.concatenate(pts).astype(f32)


def random_pairs(n, seed, well_shaped=False):
    """(triangle, point) pairs for the cull's lemma: offsets 0, 100, 1024, 4096; sizes 1e-3 .. 100 (log
    uniform); a tenth slivers (AC = s AB + 1e-5 noise), a tenth degenerate (zero edge, equal or opposite
    edges); points from 0 to 1000 sizes away from a point of the triangle.  well_shaped: edge ratio and
    the sine of the angle at A within [0.2, 5] instead of slivers and degenerates."""
    rng = np.random.default_rng(seed)
    off = rng.choice([0.0, 100.0, 1024.0, 4096.0], (n, 1))
    size = 10.0 ** rng.uniform(-3, 2, (n, 1))
    A = off * rng.choice([-1.0, 1.0], (n, 3)) + rng.uniform(-1, 1, (n, 3)) * size
    AB = rng.normal(size=(n, 3))
    AB *= size / np.linalg.norm(AB, axis=1, keepdims=True)
    AC = rng.normal(size=(n, 3))
    AC *= size * rng.uniform(0.25, 4.0, (n, 1)) / np.linalg.norm(AC, axis=1, keepdims=True)
    if not well_shaped:
        kind = rng.random(n)
        sl = kind < 0.1
        AC[sl] = rng.uniform(-2, 2, (sl.sum(), 1)) * AB[sl] + 1e-5 * rng.normal(size=(sl.sum(), 3))
        dg = (kind >= 0.1) & (kind < 0.2)
        which = rng.integers(0, 4, n)
        AB[dg & (which == 0)] = 0.0
        AC[dg & (which == 1)] = AB[dg & (which == 1)]
        AC[dg & (which == 2)] = -0.5 * AB[dg & (which == 2)]
        AC[dg & (which == 3)] = 0.0
    w = rng.random((n, 2))
    w[w.sum(1) > 1] = 1 - w[w.sum(1) > 1]
    snap = rng.random(n) < 0.2  # exactly on corners and edge midpoints
    w[snap] = np.array([(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5)])[rng.integers(0, 6, int(snap.sum()))]
    on = A + w[:, :1] * AB + w[:, 1:] * AC
    far = np.where(rng.random((n, 1)) < 0.15, 0.0, 10.0 ** rng.uniform(-4, 3, (n, 1)))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # a quarter: straight along an axis from a corner, where the box distance is the distance or close to it
    tight = rng.random(n) < 0.25
    corner = np.array([(0, 0), (1, 0), (0, 1)])[rng.integers(0, 3, n)]
    on[tight] = (A + corner[:, :1] * AB + corner[:, 1:] * AC)[tight]
    axis = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], (n, 1))
    d[tight] = axis[tight]
    p = on + d * far * size
    tri = np.concatenate([A, AB, AC], 1).astype(f32)
    if well_shaped:
        a, b, c = tri[:, :3].astype(np.float64), tri[:, 3:6].astype(np.float64), tri[:, 6:].astype(np.float64)
        lb, lc = np.linalg.norm(b, axis=1), np.linalg.norm(c, axis=1)
        sine = np.linalg.norm(np.cross(b, c), axis=1) / (lb * lc)
        keep = (lc / lb >= 0.2) & (lc / lb <= 5) & (sine >= 0.2)
        return tri[keep], p.astype(f32)[keep]
    return tri, p.astype(f32)


def hull_lb(tri, p):
    """float32: the box distance lb of p to the hull of A, fl(A + AB), fl(A + AC) as the walk computes it
    (dx = max(0, mn.x - p.x, p.x - mx.x), lb = dx*dx + dy*dy + dz*dz), and M, the largest |coordinate| of
    p and the box."""
    A = tri[:, :3]
    corners = np.stack([A, A + tri[:, 3:6], A + tri[:, 6:]], 1)
    assert corners.dtype == f32
    mn, mx = corners.min(1), corners.max(1)
    d = np.maximum(np.maximum(f32(0), mn - p), p - mx)
    sq = d * d
    lb = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    assert lb.dtype == f32
    M = np.maximum(np.abs(p).max(1), np.maximum(np.abs(mn).max(1), np.abs(mx).max(1)))
    return lb, M


def closest_d2_f64(tri, p):
    """The squared distance from p to the triangle in float64: the minimum over the face's interior
    projection (where it falls inside) and the three edges as clamped segments."""
    t = tri.astype(np.float64)
    A, AB, AC = t[:, :3], t[:, 3:6], t[:, 6:]
    B, C = A + AB, A + AC
    p = p.astype(np.float64)

    def seg(P, Q):
        e = Q - P
        ee = (e * e).sum(1)
        s = np.clip(np.where(ee > 0, ((p - P) * e).sum(1) / np.where(ee > 0, ee, 1), 0.0), 0, 1)
        r = p - (P + s[:, None] * e)
        return (r * r).sum(1)

    best = np.minimum(np.minimum(seg(A, B), seg(A, C)), seg(B, C))
    n = np.cross(AB, AC)
    nn = (n * n).sum(1)
    ok = nn > 0
    ap = p - A
    nn1 = np.where(ok, nn, 1)
    u = (np.cross(ap, AC) * n).sum(1) / nn1
    v = (np.cross(AB, ap) * n).sum(1) / nn1
    inside = ok & (u >= 0) & (v >= 0) & (u + v <= 1)
    h = (ap * n).sum(1)
    return np.where(inside, np.minimum(best, h * h / nn1), best)


# ---- a query's expected answers ------------------------------------------------------------------------
class Candidates:
    """The candidate set of cfg's scene (host-only accessors): per kind its records for mrt_point_distance."""

    def __init__(self, cfg, lights_only=False):
        import mobileraytracer_amd as m
        lkind, lgeom, _ = m.scene_lights(cfg)
        self.sets = []  # (kind, records (count, width), candidate mask)
        if not lights_only:
            planes = m.scene_planes(cfg)[0].reshape(-1, 6)
            spheres = m.scene_spheres(cfg)[0].reshape(-1, 4)
            tris = m.scene_triangles(cfg)[0].reshape(-1, 9)
            self.sets += [(PLANE, planes, np.ones(len(planes), bool)), (SPHERE, spheres, np.ones(len(spheres), bool)),
                          (TRIANGLE, tris, np.ones(len(tris), bool))]
        self.sets.append((LIGHT, lgeom.reshape(-1, 9), lkind == 1))  # point lights are never candidates
        self.count = {kind: len(rec) for kind, rec, _ in self.sets}

    def expected(self, points, max_dist=None, src=None, chunk=256):
        """kind, index, dist2, point, bary as the header defines them."""
        import mobileraytracer_amd as m
        points = np.ascontiguousarray(points, f32)
        n = len(points)
        if max_dist is None:
            bound2 = np.full(n, np.inf, f32)
        else:
            md = np.asarray(max_dist, f32)
            with np.errstate(all="ignore"):
                bound2 = np.where(md > 0, md * md, f32(0)).astype(f32)
        best = bound2.copy()
        kind, index = np.zeros(n, np.int32), np.full(n, -1, np.int32)
        for k, rec, cand in self.sets:
            T = len(rec)
            if T == 0 or not cand.any():
                continue
            for a in range(0, n, chunk):
                pts = points[a:a + chunk]
                c = len(pts)
                d2 = m.point_distance(k, np.tile(rec, (c, 1)), np.repeat(pts, T, 0))[0].reshape(c, T)
                ok = (d2 < best[a:a + c, None]) & cand[None, :]  # (a NaN d2: never below)
                if src is not None and k in (PLANE, TRIANGLE):
                    s = np.asarray(src)[a:a + c]
                    named = (s[:, 0] == k) & (s[:, 1] >= 0) & (s[:, 1] < T)
                    ok[np.nonzero(named)[0], s[named, 1]] = False
                d2 = np.where(ok, d2, np.inf)
                j = d2.argmin(1)  # the first of equal minima: the lower input index
                won = ok[np.arange(c), j]  # (kinds arrive in order: an equal d2 of a later kind loses)
                rows = a + np.nonzero(won)[0]
                best[rows], kind[rows], index[rows] = d2[won, j[won]], k, j[won]
        out = {"kind": kind, "index": index, "dist2": best, "point": np.zeros((n, 3), f32), "bary": np.zeros((n, 2), f32)}
        for k, rec, _ in self.sets:
            rows = np.nonzero(kind == k)[0]
            if len(rows):
                d2, q, uv = m.point_distance(k, rec[index[rows]], points[rows])
                assert np.array_equal(bits(d2), bits(best[rows]))
                out["point"][rows], out["bary"][rows] = q, uv
        return out


def assert_same(got, want, what="", fields=FIELDS):
    for f in fields:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        if g.dtype == f32:
            g, w = bits(g), bits(w)
        bad = (g != w).reshape(len(g), -1).any(1)
        assert not bad.any(), "%s field %s differs in %d of %d points, first %d: got %s want %s" % (
            what, f, bad.sum(), len(g), np.argmax(bad), got[f][np.argmax(bad)], want[f][np.argmax(bad)])
