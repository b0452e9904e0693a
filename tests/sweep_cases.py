"""Pairs, sweeps and host-side expectations for the sweep query (tests only).

`Lists.expected` builds a query's answer as the header defines it, from mrt_sphere_sweep over the scene
accessors and nothing else: the function's t on every (candidate, ray) pair, the mask hit and t < bound (the
`src` pair out), the answer by a lexsort on (t bits, kind, input index), every other field from that pair's own
record, a miss's padding.  Nothing of the walk is restated here.

`first_contact_f64` is the contract's yardstick: the closed-form sweep in float64 with exact feature
membership, on the stored float32 corners A, fl(A + AB), fl(A + AC); `distance_f64` the exact distance.
"""
import numpy as np

import nearest_cases as N
import neighbour_cases as NB
import overlap_cases as OC

f32 = np.float32
EPS = 2.0 ** -24
G = 64.0        # kSweepG: the measured g of the two-sided contract (the tests pin 4 G)
SWEEP_K = 32.0  # kSweepK: the validation slack, in eps M
NEAREST_K = 32.0  # kNearestK: the nearest-point lemma's k
PLANE, SPHERE, TRIANGLE, LIGHT = N.PLANE, N.SPHERE, N.TRIANGLE, N.LIGHT
FIELDS = ("hit", "kind", "index", "t", "centre", "point", "bary")  # every field but `tests`
WIDTHS = {"hit": 1, "kind": 1, "index": 1, "t": 1, "centre": 3, "point": 3, "bary": 2, "tests": 1}
OFFSETS = OC.OFFSETS
bits = N.bits


# ---- the contract's pairs ------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(rng, u):
    v = np.cross(u, _unit(rng, len(u)))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _aimed(rng, on, away, size, r, p_away):
    """Sweeps (o, d) of spheres of radius r aimed at the points `on` of a surface: the path passes `on` at
    the lateral distance k r - a share well inside (k < 0.9), a share grazing (|k - 1| = 1e-7 .. 1e-1, offset
    along `away`, the direction off the surface), a share passing outside - from 0 .. 100 r back; a tenth
    start in contact, one in forty has d = 0 and the share p_away moves away."""
    n = len(on)
    u = _unit(rng, n)
    mode = rng.random(n)
    lat = _perp(rng, u)
    out = away - (away * u).sum(1, keepdims=True) * u
    ln = np.linalg.norm(out, axis=1, keepdims=True)
    graze = (mode >= 0.4) & (mode < 0.7) & (ln[:, 0] > 1e-3)
    lat[graze] = (out / np.where(ln > 0, ln, 1))[graze]
    k = np.where(mode < 0.4, rng.uniform(0, 0.9, n),
                 np.where(mode < 0.7, 1.0 + rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-7, -1, n),
                          rng.uniform(1.05, 6.0, n)))[:, None]
    back = r * 10.0 ** rng.uniform(-1, 2, (n, 1))
    o = on + lat * k * r - u * back
    touching = rng.random(n) < 0.1
    o[touching] = (on + _unit(rng, n) * r * rng.uniform(0, 1.2, (n, 1)))[touching]
    d = u * (back + size) * 10.0 ** rng.uniform(-0.5, 0.5, (n, 1))
    still = rng.random(n) < 0.025
    d[still] = 0.0
    awayish = rng.random(n) < p_away
    d[awayish] = -d[awayish]
    return o, d


def triangle_sweeps(n, seed):
    """(triangle, sweep) pairs spread over OFFSETS: the triangles of overlap_cases.triangle_pairs (sizes
    1e-3 .. 2, a tenth slivers, a twentieth degenerate), r = 1e-3 .. 1 sizes, aimed at a point of the triangle
    (half of them at an edge or a corner, where grazing contacts are) as _aimed describes."""
    rng = np.random.default_rng(seed)
    per = n // len(OFFSETS)
    tri = np.concatenate([OC.triangle_pairs(per, seed + 1 + k, off)[0] for k, off in enumerate(OFFSETS)])
    t = tri.astype(np.float64)
    A, AB, AC = t[:, :3], t[:, 3:6], t[:, 6:]
    size = np.maximum(np.linalg.norm(AB, axis=1), np.linalg.norm(AC, axis=1))[:, None]
    size = np.where(size > 0, size, 10.0 ** rng.uniform(-3, 0.3, (n, 1)))
    w = rng.random((n, 2))
    w[w.sum(1) > 1] = 1 - w[w.sum(1) > 1]
    rim = rng.random(n) < 0.5  # on an edge or a corner
    w[rim, rng.integers(0, 2, int(rim.sum()))] = 0.0
    corner = rim & (rng.random(n) < 0.3)
    w[corner] = np.array([(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)])[rng.integers(0, 3, int(corner.sum()))]
    on = A + w[:, :1] * AB + w[:, 1:] * AC
    away = on - (A + (AB + AC) / 3.0)
    inner = ~rim
    nrm = np.cross(AB, AC)
    away[inner] = nrm[inner] * rng.choice([-1.0, 1.0], (int(inner.sum()), 1))
    r = size * 10.0 ** rng.uniform(-3, 0, (n, 1))
    r[rng.random(n) < 0.01] = 0.0
    o, d = _aimed(rng, on, away, size, r, 0.12)
    return tri, np.concatenate([o, d, r], 1).astype(f32)


def plane_sweeps(n, seed):
    """(plane, sweep) pairs over OFFSETS: unit normals (a third along an axis), r = 1e-3 .. 2."""
    rng = np.random.default_rng(seed)
    prims = OC.plane_pairs(n, seed + 1)[0]
    p = prims.astype(np.float64)
    size = 10.0 ** rng.uniform(-3, np.log10(2.0), (n, 1))
    tng = _perp(rng, p[:, :3] / np.linalg.norm(p[:, :3], axis=1, keepdims=True))
    on = p[:, 3:6] + tng * size * rng.uniform(0, 4, (n, 1))
    r = size * 10.0 ** rng.uniform(-3, 0, (n, 1))
    o, d = _aimed(rng, on, p[:, :3] * rng.choice([-1.0, 1.0], (n, 1)), size, r, 0.4)
    return prims, np.concatenate([o, d, r], 1).astype(f32)


def sphere_sweeps(n, seed):
    """(sphere, sweep) pairs over OFFSETS: radii 1e-3 .. 2, r = 1e-3 .. 1 radii, from outside and inside."""
    rng = np.random.default_rng(seed)
    prims = OC.sphere_pairs(n, seed + 1)[0]
    p = prims.astype(np.float64)
    R = np.sqrt(p[:, 3:4])
    nr = _unit(rng, n)
    on = p[:, :3] + nr * R
    r = R * 10.0 ** rng.uniform(-3, 0, (n, 1))
    o, d = _aimed(rng, on, nr * rng.choice([-1.0, 1.0], (n, 1)), R, r, 0.4)
    return prims, np.concatenate([o, d, r], 1).astype(f32)


PAIRS = {TRIANGLE: triangle_sweeps, PLANE: plane_sweeps, SPHERE: sphere_sweeps}


# ---- the float64 yardstick -------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(1)


def _seg_dist2(p, a, e):
    ee = _dot(e, e)
    s = np.clip(np.where(ee > 0, _dot(p - a, e) / np.where(ee > 0, ee, 1), 0.0), 0.0, 1.0)
    q = a + e * s[:, None]
    return _dot(p - q, p - q)


def distance_f64(kind, prims, p):
    """The exact distance from the points p (n, 3) to the primitives, on the stored float32 values."""
    prims = np.ascontiguousarray(prims, f32)
    p = np.asarray(p, np.float64)
    f = prims.astype(np.float64)
    if kind == PLANE:
        return np.abs(_dot(f[:, :3], p - f[:, 3:6])) / np.linalg.norm(f[:, :3], axis=1)
    if kind == SPHERE:
        return np.abs(np.linalg.norm(p - f[:, :3], axis=1) - np.sqrt(f[:, 3]))
    P0, P1, P2 = (x.astype(np.float64) for x in OC.corners32(prims))
    e0, e1 = P1 - P0, P2 - P0
    d2 = np.minimum(np.minimum(_seg_dist2(p, P0, e0), _seg_dist2(p, P0, e1)), _seg_dist2(p, P1, P2 - P1))
    n = np.cross(e0, e1)
    nn = _dot(n, n)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1)
    ap = p - P0
    # barycentrics of the projection: inside the face, the distance is the plane's
    b1 = _dot(np.cross(ap, e1), n) / nn1
    b2 = _dot(np.cross(e0, ap), n) / nn1
    inside = ok & (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1)
    return np.sqrt(np.where(inside, np.minimum(d2, _dot(n, ap) ** 2 / nn1), d2))


def _roots(m, d, rad2):
    """Both parameters at which -m + d s is at distance sqrt(rad2) from the origin (NaN: none)."""
    dd = _dot(d, d)
    ok = dd > 0
    dd1 = np.where(ok, dd, 1)
    tca = _dot(m, d) / dd1
    w = m - d * tca[:, None]
    disc = rad2 - _dot(w, w)
    with np.errstate(invalid="ignore"):
        h = np.sqrt(np.where(ok & (disc >= 0), disc / dd1, np.nan))
    return tca - h, tca + h


def first_contact_f64(kind, prims, rays, radius=None):
    """The exact first-contact time of the spheres (radius: rays[:, 6], or the given ones; a negative radius
    touches nothing) swept along rays (o, d) against the primitives; +inf: never."""
    prims = np.ascontiguousarray(prims, f32)
    ry = np.asarray(rays, np.float64)
    o, d = ry[:, :3], ry[:, 3:6]
    rad = ry[:, 6] if radius is None else np.asarray(radius, np.float64)
    n = len(ry)
    best = np.full(n, np.inf)
    live = rad >= 0
    rad = np.where(live, rad, 0.0)
    tol = 1e-9

    def offer(t, member):
        nonlocal best
        with np.errstate(invalid="ignore"):
            ok = member & (t >= 0) & (t < best)
        best = np.where(ok, t, best)

    f = prims.astype(np.float64)
    if kind == PLANE:
        nl = np.linalg.norm(f[:, :3], axis=1)
        s0, nd = _dot(f[:, :3], o - f[:, 3:6]) / nl, _dot(f[:, :3], d) / nl
        with np.errstate(divide="ignore", invalid="ignore"):
            for sign in (1.0, -1.0):
                offer((sign * rad - s0) / nd, nd != 0)
    elif kind == SPHERE:
        R = np.sqrt(f[:, 3])
        m = f[:, :3] - o
        for rr in (R + rad, R - rad):
            for t in _roots(m, d, np.where(rr >= 0, rr * rr, -1.0)):
                offer(t, rr >= 0)
    else:
        P0, P1, P2 = (x.astype(np.float64) for x in OC.corners32(prims))
        e0, e1 = P1 - P0, P2 - P0
        nrm = np.cross(e0, e1)
        nn = _dot(nrm, nrm)
        has = nn > 0
        nn1 = np.where(has, nn, 1)
        nl = np.sqrt(nn1)
        s0, nd = _dot(nrm, o - P0) / nl, _dot(nrm, d) / nl
        with np.errstate(divide="ignore", invalid="ignore"):
            for sign in (1.0, -1.0):
                t = (sign * rad - s0) / nd
                ap = o + d * np.where(np.isfinite(t), t, 0.0)[:, None] - P0
                b1, b2 = _dot(np.cross(ap, e1), nrm) / nn1, _dot(np.cross(e0, ap), nrm) / nn1
                offer(t, has & (nd != 0) & (b1 >= -tol) & (b2 >= -tol) & (b1 + b2 <= 1 + tol))
        for a, e in ((P0, e0), (P0, e1), (P1, P2 - P1)):
            ee = _dot(e, e)
            ee1 = np.where(ee > 0, ee, 1)
            m = a - o
            mp = m - e * (_dot(m, e) / ee1)[:, None]
            dp = d - e * (_dot(d, e) / ee1)[:, None]
            for t in _roots(mp, dp, rad * rad):
                c = o + d * np.where(np.isfinite(t), t, 0.0)[:, None]
                s = _dot(c - a, e) / ee1
                offer(t, (ee > 0) & (s >= -tol) & (s <= 1 + tol))
        for a in (P0, P1, P2):
            for t in _roots(a - o, d, rad * rad):
                offer(t, np.ones(n, bool))
    start = distance_f64(kind, prims, o) <= rad
    best = np.where(start, 0.0, best)
    return np.where(live, best, np.inf)


def centre64(rays, t):
    """c(t) in float64 on the stored floats (t finite)."""
    ry = np.asarray(rays, np.float64)
    return ry[:, :3] + ry[:, 3:6] * np.asarray(t, np.float64)[:, None]


def scale_of(kind, prims, rays, centre):
    """M: the largest |coordinate| of the start, the given centres (non-finite rows ignored), the primitive's
    points (a sphere: its radius too) and r."""
    prims = np.ascontiguousarray(prims, f32)
    ry = np.asarray(rays, np.float64)
    c = np.where(np.isfinite(centre), centre, 0.0)
    m = np.maximum(np.maximum(np.abs(ry[:, :3]).max(1), np.abs(c).max(1)), np.abs(ry[:, 6]))
    if kind in (TRIANGLE, LIGHT):
        for P in OC.corners32(prims):
            m = np.maximum(m, np.abs(P.astype(np.float64)).max(1))
    elif kind == PLANE:
        m = np.maximum(m, np.abs(prims[:, 3:6].astype(np.float64)).max(1))
    else:
        m = np.maximum(m, np.maximum(np.abs(prims[:, :3].astype(np.float64)).max(1), np.sqrt(prims[:, 3].astype(np.float64))))
    return m


def cull_radius(r, mr):
    """sweepCullR of the header, in float64: (r + (kSweepK + 2 kNearestK + 4) eps 4 Mr) (1 + 2^-19)."""
    return (r + (SWEEP_K + 2 * NEAREST_K + 4) * EPS * 4.0 * mr) * (1.0 + 2.0 ** -19)


# ---- sweeps for a scene ----------------------------------------------------------------------------------
def scene_sweeps(geom, n, seed, extent):
    """n sweeps (a multiple of 6) about the triangles `geom` (count, 3, 3: A, AB, AC), (n, 7) rays and (n,)
    bounds: long diagonal sweeps through the scene box, axis-parallel sweeps (two zero components of d), short
    sweeps from near the surface, starts in contact, d = 0, and radii from 0 to the scene's size.  The bounds:
    half unbounded (+inf), a quarter the pair's own least t (mrt_sphere_sweep) nudged one ulp down or up so
    that the contact falls just outside or just inside, a quarter half or twice that t (random where there is
    none)."""
    rng = np.random.default_rng(seed)
    per = n // 6
    c = NB.corners_of(geom)
    lo, hi = c.min(0).astype(np.float64), c.max(0).astype(np.float64)
    flat = geom.reshape(-1, 9)
    parts = []
    a = rng.uniform(lo - 0.5 * extent, hi + 0.5 * extent, (per, 3))  # long diagonals, through the box
    b = rng.uniform(lo, hi, (per, 3))
    parts.append((a, (b - a) * rng.uniform(0.5, 2.0, (per, 1)), extent * 10.0 ** rng.uniform(-1.5, -0.5, (per, 1))))
    a = rng.uniform(lo - 0.25 * extent, hi + 0.25 * extent, (per, 3))  # axis-parallel
    d = np.zeros((per, 3))
    d[np.arange(per), rng.integers(0, 3, per)] = rng.choice([-1.0, 1.0], per) * extent * rng.uniform(0.5, 2.0, per)
    parts.append((a, d, extent * 10.0 ** rng.uniform(-1.5, -0.5, (per, 1))))
    a = NB.surface_points(flat, per, rng, 0.1 * extent)  # short sweeps from near the surface
    parts.append((a, _unit(rng, per) * extent * 10.0 ** rng.uniform(-1.5, -0.5, (per, 1)), extent * 10.0 ** rng.uniform(-3, -1, (per, 1))))
    r = extent * 10.0 ** rng.uniform(-2.5, -1, (per, 1))  # starts in contact
    a = NB.surface_points(flat, per, rng, 0.0) + _unit(rng, per) * r * rng.uniform(0, 1.0, (per, 1))
    parts.append((a, _unit(rng, per) * extent, r))
    a = NB.surface_points(flat, per, rng, 0.05 * extent)  # d = 0, touching and not
    parts.append((a, np.zeros((per, 3)), extent * 10.0 ** rng.uniform(-3, -0.5, (per, 1))))
    a = rng.uniform(lo - extent, hi + extent, (per, 3))  # radii 0, and up to the scene's size
    r = np.where(rng.random((per, 1)) < 0.5, 0.0, extent * 10.0 ** rng.uniform(-1, 0.3, (per, 1)))
    parts.append((a, _unit(rng, per) * extent * 3.0, r))
    rays = np.concatenate([np.concatenate(p, 1) for p in parts]).astype(f32)
    assert len(rays) == n
    return rays


def bounds_for(lists, rays, seed, times=None):
    """Bounds as scene_sweeps describes, from the candidates' own times (times: lists.times(rays), if at hand)."""
    rng = np.random.default_rng(seed)
    t, hit = lists.times(rays) if times is None else times
    least = np.where(lists.valid[None, :] & hit, t, np.inf).min(1).astype(f32)
    n = len(rays)
    mode = np.arange(n) % 4 // 2 * (np.arange(n) % 4 - 1)  # 0, 0, 1, 2
    nudged = np.where(rng.random(n) < 0.5, np.nextafter(least, f32(np.inf)), least)  # just inside / exactly at (outside)
    with np.errstate(invalid="ignore"):
        rnd = np.where(np.isfinite(least) & (least > 0), least * rng.choice([0.5, 2.0], n), 10.0 ** rng.uniform(-2, 0.5, n)).astype(f32)
    return np.where(mode == 0, f32(np.inf), np.where(mode == 1, nudged, rnd)).astype(f32)


# ---- a query's expected answers ------------------------------------------------------------------------
def bound_of(n, max_t):
    if max_t is None:
        return np.full(n, np.inf, f32)
    b = np.asarray(max_t, f32)
    with np.errstate(invalid="ignore"):
        return np.where(b > 0, b, f32(0)).astype(f32)


class Lists:
    """The candidates of cfg's scene as columns in (kind, input index) order, and the expected answers."""

    def __init__(self, cfg, lights_only=False):
        nb = NB.Lists(cfg, lights_only)
        self.rec, self.kind, self.index, self.valid, self.first = nb.rec, nb.kind, nb.index, nb.valid, nb.first
        self.fixed = nb.fixed

    def times(self, rays, chunk=256):
        """mrt_sphere_sweep of every (candidate, ray) pair: hit (n, candidates) bool and t float32."""
        import mobileraytracer_amd as m
        rays = np.ascontiguousarray(rays, f32)
        t = np.empty((len(rays), len(self.kind)), f32)
        hit = np.zeros(t.shape, bool)
        for k, rec in self.rec.items():
            T, c0 = len(rec), self.first[k]
            for a in range(0, len(rays), chunk):
                ry = rays[a:a + chunk]
                h, tt = m.sphere_sweep(k, np.tile(rec, (len(ry), 1)), np.repeat(ry, T, 0))[:2]
                hit[a:a + chunk, c0:c0 + T] = h.reshape(len(ry), T) != 0
                t[a:a + chunk, c0:c0 + T] = tt.reshape(len(ry), T)
        return t, hit

    def expected(self, rays, max_t=None, src=None, times=None):
        """hit, kind, index, t, centre, point, bary as the header defines them (times: times(rays), if at hand)."""
        import mobileraytracer_amd as m
        rays = np.ascontiguousarray(rays, f32)
        n = len(rays)
        t, hit = self.times(rays) if times is None else times
        bound = bound_of(n, max_t)
        with np.errstate(invalid="ignore"):
            ok = hit & (t < bound[:, None]) & self.valid[None, :]
        if src is not None:
            s = np.asarray(src)
            for k in (PLANE, TRIANGLE):
                if k in self.rec:
                    rows = np.nonzero((s[:, 0] == k) & (s[:, 1] >= 0) & (s[:, 1] < len(self.rec[k])))[0]
                    ok[rows, self.first[k] + s[rows, 1]] = False
        assert not np.signbit(t[ok]).any()  # (so the bits order as the values do)
        key = np.where(ok, bits(t).astype(np.int64), np.int64(1) << 40)
        order = np.lexsort((np.broadcast_to(self.index, key.shape), np.broadcast_to(self.kind, key.shape), key), axis=1)
        top = order[:, 0]
        rows = np.arange(n)
        held = ok[rows, top]
        out = {"hit": held.astype(np.int32), "kind": np.where(held, self.kind[top], 0).astype(np.int32),
               "index": np.where(held, self.index[top], -1).astype(np.int32),
               "t": np.where(held, t[rows, top], bound).astype(f32),
               "centre": np.zeros((n, 3), f32), "point": np.zeros((n, 3), f32), "bary": np.zeros((n, 2), f32)}
        for kind, rec in self.rec.items():
            i = np.nonzero(held & (out["kind"] == kind))[0]
            if len(i):
                h, tt, c, q, uv = m.sphere_sweep(kind, rec[out["index"][i]], rays[i])
                assert h.all() and np.array_equal(bits(tt), bits(out["t"][i]))
                out["centre"][i], out["point"][i], out["bary"][i] = c, q, uv
        return out


def rows_of(want, rows):
    return {f: x[rows] for f, x in want.items()}


def assert_same(got, want, what="", fields=FIELDS):
    """Integers as they are, floats as bits (nearest_cases.assert_same)."""
    N.assert_same(got, want, what, fields=[f for f in fields if f in want and f in got])
