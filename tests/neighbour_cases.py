"""Scenes, points and host-side expectations for the neighbour query (tests only).

`Lists.expected` builds a query's answer as the header defines it, from mrt_point_distance over the scene
accessors and nothing else: d2 of every (candidate, point) pair, the mask d2 < bound2 (NaN out, the `src`
pair out), count = the mask's sum, the list by a lexsort on (d2 bits, kind, input index), point and bary
from a second mrt_point_distance call on the chosen pairs, then the padding.  No formula of the distance
functions and nothing of the walk is restated here.

The scene writers repeat the recipes of the nearest-point tests (a 300-triangle soup, sheets of unit quads).
"""
import os

import numpy as np

import nearest_cases as N
import shape_scenes as S

f32 = np.float32
PLANE, SPHERE, TRIANGLE, LIGHT = N.PLANE, N.SPHERE, N.TRIANGLE, N.LIGHT
FIELDS = ("count", "kind", "index", "dist2", "point", "bary")  # every field but `tests`
LIST_FIELDS = FIELDS[1:]
WIDTHS = {"count": 0, "kind": 1, "index": 1, "dist2": 1, "point": 3, "bary": 2, "tests": 0}  # 0: one per point
K_MAX = 16
bits = N.bits


# ---- scenes ------------------------------------------------------------------------------------------
def obj_cfg(files, **kw):
    import mobileraytracer_amd as m
    return m.Config(width=16, height=16, shader=1, sceneIndex=-1, objFilePath=files[0], mtlFilePath=files[1],
                    camFilePath=files[2], **kw)


def write_mesh(path, name, tris=(), quads=(), light=None):
    os.makedirs(path, exist_ok=True)
    obj, mtl, cam = (os.path.join(path, "%s.%s" % (name, e)) for e in ("obj", "mtl", "cam"))
    with open(mtl, "w") as f:
        f.write("newmtl m\nKd 0.5 0.5 0.5\nKs 0 0 0\n\nnewmtl light\nKd 0 0 0\nKs 0 0 0\nKe 4 4 4\n")
    mesh = S._Mesh()
    for t in tris:
        mesh.tri("m", *t)
    for q in quads:
        mesh.quad("m", *q)
    if light is not None:
        mesh.quad("light", *light)
    mesh.write(obj, os.path.basename(mtl))
    with open(cam, "w") as f:
        f.write("t perspective\np 0.5 0.5 -4\nl 0.5 0.5 0\nu 0 1 0\nf 45 45\n")
    return obj, mtl, cam


def soup(path, name, offset, size, seed=31):
    """300 random triangles of about `size` with their centres in the unit cube at `offset`, and an
    emissive quad above it (two area lights)."""
    rng = np.random.default_rng(seed)
    c = offset + rng.random((300, 1, 3))
    v = (c + size * rng.normal(size=(300, 3, 3))).astype(f32)
    lo, hi = f32(offset - 0.5), f32(offset + 1.5)
    light = [(lo, hi, lo), (hi, hi, lo), (hi, hi, hi), (lo, hi, hi)]
    return write_mesh(path, name, tris=[tuple(map(tuple, t)) for t in v], light=light)


FAR_LIGHT = [(0, 0, 64), (1, 0, 64), (1, 1, 64), (0, 1, 64)]  # (a scene needs a light; this one is far from every point)


def sheet_quads(n, z):
    return [((i, j, z), (i + 1, j, z), (i + 1, j + 1, z), (i, j + 1, z)) for j in range(n) for i in range(n)]


def surface_points(geom, k, rng, jitter):
    """k points within `jitter` of random surface points of the triangles (A, AB, AC rows)."""
    t = geom.reshape(-1, 9)[rng.integers(0, len(geom), k)].astype(np.float64)
    w = rng.random((k, 2))
    w[w.sum(1) > 1] = 1 - w[w.sum(1) > 1]
    return t[:, :3] + w[:, :1] * t[:, 3:6] + w[:, 1:] * t[:, 6:] + rng.uniform(-jitter, jitter, (k, 3))


def corner_points(geom, k, rng):
    """k points exactly on corners and edge midpoints (as float32 computes them)."""
    t = geom.reshape(-1, 9)[rng.integers(0, len(geom), k)]
    w = np.array([(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5)], f32)[rng.integers(0, 6, k)]
    with np.errstate(invalid="ignore"):  # (a non-finite triangle: the caller drops its points)
        return (t[:, :3] + t[:, 3:6] * w[:, :1]) + t[:, 6:] * w[:, 1:]


def corners_of(geom):
    return np.concatenate([geom[:, 0], geom[:, 0] + geom[:, 1], geom[:, 0] + geom[:, 2]])


def soup_points(geom, per, near, seed=32):
    """3 * per points: in a box twice the scene's, within `near` of the surface, exactly on corners."""
    rng = np.random.default_rng(seed)
    c = corners_of(geom)
    lo, hi = c.min(0).astype(np.float64), c.max(0).astype(np.float64)
    return np.concatenate([rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (per, 3)),
                           surface_points(geom, per, rng, near), corner_points(geom, per, rng)]).astype(f32)


def builtin_points(cands, n, seed):
    """Uniform points in a box about the scene's finite primitives, and points near each kind's surfaces
    (found with mrt_point_distance's nearest point: no geometry is restated)."""
    import mobileraytracer_amd as m
    rng = np.random.default_rng(seed)
    rec = {k: r[c] for k, r, c in cands.sets}
    anchors = [rec[SPHERE][:, :3]] if len(rec[SPHERE]) else []
    for k in (TRIANGLE, LIGHT):
        if len(rec[k]):
            anchors += [rec[k][:, :3], rec[k][:, :3] + rec[k][:, 3:6], rec[k][:, :3] + rec[k][:, 6:]]
    a = np.concatenate(anchors).astype(np.float64)
    lo, hi = a.min(0) - 1, a.max(0) + 1
    parts = [rng.uniform(lo, hi, (n // 2, 3)).astype(f32)]
    kinds = [k for k in (PLANE, SPHERE, TRIANGLE, LIGHT) if len(rec[k])]
    per = (n - n // 2) // len(kinds)
    for k in kinds:
        seeds = rng.uniform(lo, hi, (per, 3)).astype(f32)
        q = m.point_distance(k, rec[k][rng.integers(0, len(rec[k]), per)], seeds)[1]
        parts.append((q + rng.uniform(-1e-3, 1e-3, (per, 3))).astype(f32))
    pts = np.concatenate(parts)
    return np.concatenate([pts, rng.uniform(lo, hi, (n - len(pts), 3)).astype(f32)])


# ---- a query's expected answers ------------------------------------------------------------------------
def bound2_of(n, max_dist):
    if max_dist is None:
        return np.full(n, np.inf, f32)
    md = np.asarray(max_dist, f32)
    with np.errstate(all="ignore"):
        return np.where(md > 0, md * md, f32(0)).astype(f32)


class Lists:
    """The candidates of cfg's scene as columns in (kind, input index) order, and the expected lists."""

    def __init__(self, cfg, lights_only=False):
        self.cands = N.Candidates(cfg, lights_only)
        sets = [(k, rec, cand) for k, rec, cand in self.cands.sets if len(rec)]
        if not sets:  # (a scene without a light, asked for its lights: one column that is no candidate)
            sets = [(LIGHT, np.zeros((1, 9), f32), np.zeros(1, bool))]
        self.rec = {k: rec for k, rec, _ in sets}
        self.kind = np.concatenate([np.full(len(rec), k, np.int32) for k, rec, _ in sets])
        self.index = np.concatenate([np.arange(len(rec), dtype=np.int32) for _, rec, _ in sets])
        self.valid = np.concatenate([cand for _, _, cand in sets])  # (point lights are never candidates)
        self.first = {k: int(np.argmax(self.kind == k)) for k in self.rec}  # a kind's first column
        self.fixed = int((self.valid & (self.kind != TRIANGLE)).sum())  # candidates the walk meets one by one

    def distances(self, points, chunk=256):
        """d2 of every (candidate, point) pair: (n, candidates) float32."""
        import mobileraytracer_amd as m
        points = np.ascontiguousarray(points, f32)
        out = np.empty((len(points), len(self.kind)), f32)
        for k, rec in self.rec.items():
            T, c0 = len(rec), self.first[k]
            for a in range(0, len(points), chunk):
                pts = points[a:a + chunk]
                out[a:a + chunk, c0:c0 + T] = m.point_distance(k, np.tile(rec, (len(pts), 1)),
                                                               np.repeat(pts, T, 0))[0].reshape(len(pts), T)
        return out

    def accepted(self, d2, bound2, src=None):
        """The mask of accepted candidates: d2 < bound2 (false for NaN), a candidate, not the named source."""
        with np.errstate(invalid="ignore"):
            ok = (d2 < bound2[:, None]) & self.valid[None, :]
        if src is not None:
            s = np.asarray(src)
            for k in (PLANE, TRIANGLE):
                if k in self.rec:
                    rows = np.nonzero((s[:, 0] == k) & (s[:, 1] >= 0) & (s[:, 1] < len(self.rec[k])))[0]
                    ok[rows, self.first[k] + s[rows, 1]] = False
        return ok

    def expected(self, points, k, max_dist=None, src=None, d2=None, chunk=256):
        """count, kind, index, dist2, point, bary as the header defines them (d2: distances(points), if at hand)."""
        import mobileraytracer_amd as m
        points = np.ascontiguousarray(points, f32)
        n, C = len(points), len(self.kind)
        d2 = self.distances(points) if d2 is None else d2
        bound2 = bound2_of(n, max_dist)
        ok = self.accepted(d2, bound2, src)
        assert not np.signbit(d2[ok]).any()  # (so the bits order as the values do)
        count = ok.sum(1).astype(np.int32)
        top = np.zeros((n, k), np.int64)
        w = min(k, C)
        for a in range(0, n, chunk):
            key = np.where(ok[a:a + chunk], bits(d2[a:a + chunk]).astype(np.int64), np.int64(1) << 40)
            shape = key.shape
            order = np.lexsort((np.broadcast_to(self.index, shape), np.broadcast_to(self.kind, shape), key), axis=1)
            top[a:a + chunk, :w] = order[:, :w]
        held = np.arange(k)[None, :] < count[:, None]
        rows = np.arange(n)[:, None]
        out = {"count": count, "kind": np.where(held, self.kind[top], 0).astype(np.int32),
               "index": np.where(held, self.index[top], -1).astype(np.int32),
               "dist2": np.where(held, d2[rows, top], bound2[:, None]).astype(f32),
               "point": np.zeros((n, k, 3), f32), "bary": np.zeros((n, k, 2), f32)}
        assert ok[rows, top][held].all()
        for kind, rec in self.rec.items():
            i, j = np.nonzero(held & (out["kind"] == kind))
            if len(i):
                e2, q, uv = m.point_distance(kind, rec[out["index"][i, j]], points[i])
                assert np.array_equal(bits(e2), bits(out["dist2"][i, j]))
                out["point"][i, j], out["bary"][i, j] = q, uv
        return out


def cut(want, k):
    """The answer for a smaller K from the one for a larger: the count, and the first k entries."""
    return {f: (x if f == "count" else x[:, :k]) for f, x in want.items()}


def rows_of(want, rows):
    return {f: x[rows] for f, x in want.items()}


def assert_same(got, want, what="", fields=FIELDS):
    """Integers as they are, floats as bits (nearest_cases.assert_same, on lists)."""
    N.assert_same(got, want, what, fields=[f for f in fields if f in want])
