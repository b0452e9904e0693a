"""Multi-hit queries (mrt_cast_multi_hits_device): the first K hits along each ray, in order, the hit
count and the padding.  Every comparison is exact (count, kind, index, the bits of t and of u, v).

Expected lists of triangle-and-light scenes are built from the kernels' own arithmetic: t of every
(ray, triangle) pair from kat_triangle, u and v from the float32 restatement of Triangle::intersect, the
visit set from triangle_bvh's boxes with the reference slab predicate (kat_slab) applied from the root
down, then sorted by the documented order (t, kind, walk-order index).  Planes and spheres (built-in
scenes only: an OBJ holds none) are restated in float32 from the scene accessors and pinned under the
Naive accelerator, which tests every primitive; the BVH is then compared with Naive.

Frames are 16 x 16; outputs given to the C entry point start filled with a sentinel."""
import dataclasses
import os

import numpy as np
import pytest

import hit_scenes as H
import shape_scenes as S
from test_cast_rays_gpu import SENTINEL, bits, dev, mixed_rays
from test_hit_records_gpu import barycentrics, dot, room_cfg

pytestmark = pytest.mark.gpu

f32 = np.float32
EPS, EPS_LARGE, RAY_MAX = f32(1.0e-06), f32(1.0e-05), f32(1.0e+30)
FIELDS = ("count", "kind", "index", "t", "bary")
PLANE, SPHERE, TRIANGLE, LIGHT = 1, 2, 3, 4
NAIVE, GRID = 1, 2


# ---- the query on host arrays ------------------------------------------------------------------------
def multi(r, o, d, k, dist=None, src=None, fields=None):
    got = r.cast_multi_hits(dev(o), dev(d), k, dist=None if dist is None else dev(dist),
                            src=None if src is None else dev(src), fields=fields)
    return {f: x.cpu().numpy() for f, x in got.items()}


def assert_lists(got, want, what=""):
    for f in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = bits(g), bits(w)
        bad = (g != w).reshape(len(g), -1).any(1)
        assert not bad.any(), "%s field %s differs in %d of %d rays, first ray %d: got %s want %s" % (
            what, f, bad.sum(), len(g), np.argmax(bad), got[f][np.argmax(bad)], want[f][np.argmax(bad)])


# ---- expected lists ----------------------------------------------------------------------------------
def tri_tests(geom, o, d):
    """Every (ray, triangle (A, AB, AC)) pair: accepted at RayLengthMax and t from the kernels' own
    triTest (kat_triangle), u and v restated; arrays (n, T)."""
    import mobileraytracer_amd as m
    n, T = len(o), len(geom)
    if T == 0:
        return np.zeros((n, 0), bool), np.zeros((n, 0), f32), np.zeros((n, 0), f32), np.zeros((n, 0), f32)
    abc = np.stack([geom[:, 0], geom[:, 0] + geom[:, 1], geom[:, 0] + geom[:, 2]], 1)
    # (the triangles' coordinates are dyadic and small: (A + AB) - A is AB again)
    assert np.array_equal(abc[:, 1] - abc[:, 0], geom[:, 1]) and np.array_equal(abc[:, 2] - abc[:, 0], geom[:, 2])
    oo, dd = np.repeat(o, T, 0), np.repeat(d, T, 0)
    hit, t = m.kat_triangle(np.tile(abc.reshape(T, 9), (n, 1)), oo, dd)
    with np.errstate(all="ignore"):
        u, v = barycentrics(oo, dd, np.tile(geom, (n, 1, 1)))
    return hit.reshape(n, T).astype(bool), t.reshape(n, T), u.reshape(n, T).astype(f32), v.reshape(n, T).astype(f32)


def visited(boxes, off, cnt, o, d):
    """(n, T) by walk position: the triangle's leaf box and every ancestor's pass the reference slab
    predicate (kat_slab's out[3i]) for the ray."""
    import mobileraytracer_amd as m
    n, N = len(o), len(boxes)
    pred = m.kat_slab(np.tile(boxes, (n, 1)), np.repeat(o, N, 0), np.repeat(d, N, 0))[:, 0].reshape(n, N).astype(bool)
    vis = np.zeros((n, int(cnt[cnt > 0].sum())), bool)
    stack = [(0, pred[:, 0])]
    while stack:
        node, reach = stack.pop()
        if cnt[node] > 0:
            vis[:, off[node]:off[node] + cnt[node]] = reach[:, None]
        else:
            for c in (int(off[node]), int(off[node]) + 1):
                stack.append((c, reach & pred[:, c]))
    return vis


def plane_tests(planes, o, d):
    """leafPlanes (Plane.cpp:38-72) in float32, (n, P): tested value t, and whether it passes the
    denominator and the t < Epsilon tests."""
    n = planes[None, :, 0]
    with np.errstate(all="ignore"):
        den = dot(n, d[:, None, :])
        num = dot(n, planes[None, :, 1] - o[:, None, :])
        t = (num / den).astype(f32)
    return (~(np.abs(den) < EPS)) & ~(t < EPS), t


def sphere_tests(spheres, o, d):
    """leafSpheres (Sphere.cpp:42-81) in float32, (n, S)."""
    with np.errstate(all="ignore"):
        oc = spheres[None, :, :3] - o[:, None, :]
        dd = np.broadcast_to(d[:, None, :], oc.shape)
        proj = dot(oc, dd)
        mag = np.sqrt(dot(oc, oc))
        a = dot(dd, dd)
        bq = f32(2.0) * -proj
        c = mag * mag - spheres[None, :, 3]
        disc = bq * bq - f32(4.0) * a * c
        r = np.sqrt(disc)
        d1, d2 = -bq + r, -bq - r
        t = (np.where(d2 < d1, d2, d1) / (f32(2.0) * a)).astype(f32)
    return ~(disc < 0) & ~(t < EPS_LARGE), t


class Scene:
    """What the expected lists need of cfg's scene (host-only accessors)."""

    def __init__(self, cfg):
        import mobileraytracer_amd as m
        self.cfg = cfg
        self.geom = m.scene_triangles(cfg)[0]
        self.planes = m.scene_planes(cfg)[0]
        self.spheres = m.scene_spheres(cfg)[0]
        lkind, self.lgeom, _ = m.scene_lights(cfg)
        self.area = lkind == 1
        if len(self.geom):
            self.boxes, self.off, self.cnt, self.order = m.triangle_bvh(cfg)
            self.pos = np.empty(len(self.geom), np.int64)  # input index -> walk-order index
            self.pos[self.order] = np.arange(len(self.geom))

    def lists(self, o, d, K, tmax=None, src=None, naive=False):
        """count, kind, index, t, bary as the header states them.  naive False: the triangles of the
        visited leaves only, ties by walk-order index (the scene must hold no plane and no sphere: their
        trees have no accessor); True: every primitive, ties by input index."""
        o, d = np.asarray(o, f32), np.asarray(d, f32)
        n = len(o)
        tmax = np.full(n, RAY_MAX, f32) if tmax is None else np.asarray(tmax, f32)
        cands = []  # (kind, accepted (n, X), t, u, v, tie key per primitive)
        if naive:
            ok, t = plane_tests(self.planes, o, d)
            cands.append((PLANE, ok, t, np.zeros_like(t), np.zeros_like(t), np.arange(len(self.planes))))
            ok, t = sphere_tests(self.spheres, o, d)
            cands.append((SPHERE, ok, t, np.zeros_like(t), np.zeros_like(t), np.arange(len(self.spheres))))
        else:
            assert len(self.planes) == 0 and len(self.spheres) == 0
        hit, t, u, v = tri_tests(self.geom, o, d)
        if len(self.geom):
            if naive:
                key = np.arange(len(self.geom))
            else:
                hit = hit & visited(self.boxes, self.off, self.cnt, o, d)[:, self.pos]
                key = self.pos
            cands.append((TRIANGLE, hit, t, u, v, key))
        lhit, lt, lu, lv = tri_tests(self.lgeom, o, d)
        cands.append((LIGHT, lhit & self.area[None, :], lt, lu, lv, np.arange(len(self.lgeom))))
        out = {"count": np.zeros(n, np.int32), "kind": np.zeros((n, K), np.int32), "index": np.full((n, K), -1, np.int32),
               "t": np.repeat(tmax[:, None], K, 1), "bary": np.zeros((n, K, 2), f32)}
        for i in range(n):
            ents = []
            for kind, ok, t, u, v, key in cands:
                for j in np.nonzero(ok[i])[0]:
                    if not t[i, j] < tmax[i]:  # (a NaN t: left out)
                        continue
                    if src is not None and kind in (PLANE, TRIANGLE) and (int(src[i][0]), int(src[i][1])) == (kind, j):
                        continue
                    ents.append((t[i, j], kind, key[j], j, u[i, j], v[i, j]))
            ents.sort(key=lambda e: e[:3])
            out["count"][i] = len(ents)
            for k, e in enumerate(ents[:K]):
                out["kind"][i, k], out["index"][i, k], out["t"][i, k] = e[1], e[3], e[0]
                out["bary"][i, k] = (e[4], e[5])
        return out


def obj_cfg(files, **kw):
    import mobileraytracer_amd as m
    return m.Config(width=16, height=16, shader=1, sceneIndex=-1, objFilePath=files[0], mtlFilePath=files[1],
                    camFilePath=files[2], **kw)


# ---- the layers --------------------------------------------------------------------------------------
def write_layers(path, L, light_z=None):
    """L unit quads [0, 1]^2 at z = 1 .. L (2 L triangles) and an emissive quad (two area lights, written
    last) over the same square at z = light_z (default L + 1, behind every layer for a +z ray).  (The
    loader mirrors x: the file's x runs from 0 to -1.)"""
    os.makedirs(path, exist_ok=True)
    obj, mtl, cam = (os.path.join(path, "layers%d.%s" % (L, e)) for e in ("obj", "mtl", "cam"))
    with open(mtl, "w") as f:
        f.write("newmtl m\nKd 0.5 0.5 0.5\nKs 0 0 0\n\nnewmtl light\nKd 0 0 0\nKs 0 0 0\nKe 4 4 4\n")
    mesh = S._Mesh()
    for z in range(1, L + 1):
        mesh.quad("m", (0, 0, z), (-1, 0, z), (-1, 1, z), (0, 1, z))
    lz = L + 1 if light_z is None else light_z
    mesh.quad("light", (0, 0, lz), (-1, 0, lz), (-1, 1, lz), (0, 1, lz))
    mesh.write(obj, os.path.basename(mtl))
    with open(cam, "w") as f:
        f.write("t perspective\np -0.5 0.5 -4\nl -0.5 0.5 0\nu 0 1 0\nf 45 45\n")
    return obj, mtl, cam


def layer_rays(L):
    """+z rays in front of, between, exactly on and beside the layers, a few slanted, a few backwards."""
    xy = [(x, y) for x in (0.125, 0.25, 0.5, 0.625, 0.875) for y in (0.125, 0.375, 0.5, 0.75, 0.875)]  # (0.5, 0.5): on the diagonal
    o, d = [], []
    for x, y in xy:
        o.append((x, y, 0.0))
        d.append((0.0, 0.0, 1.0))
    for z in (1.5, 2.5, L - 0.5, L + 0.5, 1.0, 2.0, float(L), float(L + 1)):  # between, and exactly on a layer / the light
        for x, y in xy[::5]:
            o.append((x, y, z))
            d.append((0.0, 0.0, 1.0))
    for x, y in ((2.5, 0.5), (-0.5, 0.25), (0.5, 1.5), (0.25, -3.0)):  # beside the square: nothing
        o.append((x, y, 0.0))
        d.append((0.0, 0.0, 1.0))
    for x, y in xy[:3]:  # away from everything
        o.append((x, y, 0.0))
        d.append((0.0, 0.0, -1.0))
    for x, y in xy[:6]:  # slanted: leaves the square after a few layers
        o.append((x, y, 0.0))
        d.append((0.125, 0.0625, 1.0))
    o, d = np.array(o, f32), np.array(d, f32)
    assert len(o) > 64 and len(o) % 64 != 0
    return o, d


@pytest.fixture(scope="module")
def layers(tmp_path_factory):
    """Per L: the scene, its rays and the expected lists at K = 16 (the lists at a smaller K are their
    prefixes); made on first use, shared read-only."""
    path = str(tmp_path_factory.mktemp("layers"))
    cache = {}

    def get(L):
        if L not in cache:
            sc = Scene(obj_cfg(write_layers(path, L)))
            assert len(sc.geom) == 2 * L and sc.area.sum() == 2
            o, d = layer_rays(L)
            cache[L] = (sc, o, d, sc.lists(o, d, 16))
        return cache[L]
    return get


def prefix(want, K):
    """The expected lists at K from those at 16."""
    return {"count": want["count"], "kind": want["kind"][:, :K], "index": want["index"][:, :K], "t": want["t"][:, :K],
            "bary": want["bary"][:, :K]}


# ---- 1. layers: count, order, truncation, padding ----------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("L", [1, 3, 16, 17, 35])
def test_layers_count_order_truncation_and_padding(layers, L, K):
    import mobileraytracer_amd as m
    sc, o, d, want16 = layers(L)
    want = sc.lists(o, d, K) if K == 16 else prefix(want16, K)
    # (on the CPU, before any comparison: the cases are what they claim)
    front = want16["count"][:25]  # every layer and the light; both triangles of each where the ray crosses the shared diagonal
    assert set(front.tolist()) == {L + 1, 2 * (L + 1)}
    assert (want16["count"] == 0).sum() >= 7 and want16["count"].max() == 2 * (L + 1)
    with m.Renderer(sc.cfg) as r:
        got = multi(r, o, d, K)
    assert_lists(got, want, "L %d K %d" % (L, K))
    # the list in words: t ascending, the padding as stated
    n_listed = np.minimum(got["count"], K)
    for i in range(len(o)):
        k = n_listed[i]
        assert (np.diff(got["t"][i, :k]) >= 0).all()
        assert (got["kind"][i, k:] == 0).all() and (got["index"][i, k:] == -1).all()
        assert (bits(got["t"][i, k:]) == bits(RAY_MAX)).all() and (bits(got["bary"][i, k:]) == 0).all()
    # a ray that starts exactly on a layer does not list it (t < Epsilon)
    on = np.nonzero((o[:, 2] == 1.0) & (d[:, 2] > 0) & (o[:, 0] < 1))[0]
    assert len(on) and (got["t"][on, 0] >= 1.0).all() and set(got["count"][on].tolist()) <= {L, 2 * L}


# ---- 2. ties -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 16])
def test_coincident_triangles_are_listed_by_walk_order(tmp_path, K):
    import mobileraytracer_amd as m
    files = S.write_stack(str(tmp_path), 9)
    first = files[3]
    sc = Scene(obj_cfg(files[:3]))
    o = np.array([(0.125, 0.125, -9.0), (0.5, -1.0, -9.0), (-0.875, -1.625, -9.0), (0.375, 0.875, -9.0)] * 17, f32)[:67]
    d = np.tile(np.array([(0.0, 0.0, 1.0)], f32), (len(o), 1))  # (no ray on a plane of a box: x, y off the grid's 1/4s)
    want = sc.lists(o, d, K)
    with m.Renderer(sc.cfg) as r:
        got = multi(r, o, d, K)
    assert_lists(got, want, "stack 9, K %d" % K)
    copies = first + np.arange(9)
    by_walk = copies[np.argsort(sc.pos[copies])]  # the copies' input indices in ascending walk order
    m_listed = min(K, 9)
    assert (got["count"] >= 9 + 1).all()  # all nine, and the wall behind them
    assert (got["index"][:, :m_listed] == by_walk[:m_listed]).all() and (got["kind"][:, :m_listed] == TRIANGLE).all()
    assert (bits(got["t"][:, :m_listed]) == bits(f32(7.0))).all()
    # Naive lists the copies by input index: the same group in its own documented order
    with m.Renderer(dataclasses.replace(sc.cfg, accelerator=NAIVE)) as r:
        naive = multi(r, o, d, K)
    assert_lists(naive, sc.lists(o, d, K, naive=True), "stack 9, Naive, K %d" % K)
    assert (naive["index"][:, :m_listed] == copies[:m_listed]).all()
    assert assert_bvh_equals_naive(got, naive) >= len(o)  # (a tie group in every ray's list)


def test_cross_kind_ties_follow_the_reference_evaluation_order(tmp_path):
    """Bit-equal t of different kinds: plane before sphere (built-in scene 3: the ray up through the
    point where the unit sphere at (-1, 1, 6) rests on the plane y = 0, both at t = 3), triangle before
    light (an emissive quad coincident with layer 2 of the layers)."""
    import mobileraytracer_amd as m
    o = np.array([(-1.0, -3.0, 6.0)] * 3, f32)
    d = np.array([(0.0, 1.0, 0.0)] * 3, f32)
    for acc in (m.ACC_BVH, NAIVE):
        cfg = m.Config(width=16, height=16, shader=1, sceneIndex=3, accelerator=acc)
        want = Scene(cfg).lists(o, d, 4, naive=True)
        assert want["kind"][0].tolist() == [PLANE, SPHERE, 0, 0] and (bits(want["t"][0, :2]) == bits(f32(3.0))).all()
        with m.Renderer(cfg) as r:
            got = multi(r, o, d, 4)
            cast = tuple(x.cpu().numpy() for x in r.cast_rays(dev(o), dev(d)))
        assert_lists(got, want, "scene 3, accelerator %d" % acc)
        assert (cast[0] == PLANE).all() and (bits(cast[2]) == bits(got["t"][:, 0])).all()
    sc = Scene(obj_cfg(write_layers(str(tmp_path), 3, light_z=2)))
    o = np.array([(0.25, 0.5, 0.0), (0.75, 0.25, 0.0), (0.5, 0.5, 0.0)], f32)
    d = np.array([(0.0, 0.0, 1.0)] * 3, f32)
    want = sc.lists(o, d, 8)
    assert want["kind"][0].tolist() == [TRIANGLE, TRIANGLE, LIGHT, TRIANGLE, 0, 0, 0, 0]
    assert want["t"][0, :4].tolist() == [1.0, 2.0, 2.0, 3.0]
    with m.Renderer(sc.cfg) as r:
        got = multi(r, o, d, 8)
    assert_lists(got, want, "light on layer 2")


# ---- 3. entry 0 is the closest-hit query -------------------------------------------------------------
def room_rays(lo, hi):
    """2048 mixed rays in the room's box and 1001 coherent ones: a fan in through the open front."""
    o, d = mixed_rays(2048, 171, lo, hi)
    g = np.linspace(-0.4, 0.4, 1001).astype(f32)
    fan = np.stack([g, f32(0.7) * np.sin(f32(9.0) * g), np.ones_like(g)], 1)
    fan = (fan / np.linalg.norm(fan, axis=1, keepdims=True)).astype(f32)
    return np.concatenate([o, np.tile(np.array([(0.0, 0.0, -4.5)], f32), (1001, 1))]), np.concatenate([d, fan])


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    """The room (triangles and two area lights), its rays, and per accelerator the K = 8 lists and the
    closest-hit query's answers; computed once, shared read-only."""
    import mobileraytracer_amd as m
    files = H.write_room(str(tmp_path_factory.mktemp("multi_room")))
    cfg = room_cfg(files)
    sc = Scene(cfg)
    w = {"scene": sc}
    w["o"], w["d"] = room_rays(sc.boxes[0, :3], sc.boxes[0, 3:])
    for acc in (m.ACC_BVH, NAIVE):
        with m.Renderer(dataclasses.replace(cfg, accelerator=acc)) as r:
            w[acc] = (multi(r, w["o"], w["d"], 8), tuple(x.cpu().numpy() for x in r.cast_rays(dev(w["o"]), dev(w["d"]))))
    return w


def builtin_rays(scene):
    """257 rays inside the Cornell box of scene 2 (the first 32 aimed at its light quad), or above the
    plane of scene 3 among its spheres: origins well inside every primitive's box."""
    rng = np.random.default_rng(500 + scene)
    n = 257

    def through(a, b, back, m):
        """m rays from `back` behind centre a (seen from b) towards b, jittered: they cross what lies at a, then b."""
        a, b = np.asarray(a), np.asarray(b)
        start = a + (a - b) / np.linalg.norm(a - b) * back + rng.uniform(-0.02, 0.02, (m, 3))
        return start, b + rng.uniform(-0.05, 0.05, (m, 3)) - start

    if scene == 2:
        o = rng.uniform(-0.875, 0.875, (n, 3))
        d = rng.normal(size=(n, 3))
        d[:32] = np.stack([rng.uniform(-0.2, 0.2, 32), np.full(32, 0.99), rng.uniform(-0.2, 0.2, 32)], 1) - o[:32]
        o[32:64], d[32:64] = through((0.45, -0.65, 0.4), (-0.4, -0.3, 0.0), 0.45, 32)   # sphere, then sphere
        o[64:96], d[64:96] = through((-0.4, -0.3, 0.0), (0.0, 0.99, 0.0), 0.5, 32)      # sphere, then the light
    else:
        o = np.stack([rng.uniform(-3, 3, n), rng.uniform(0.25, 4, n), rng.uniform(1, 9, n)], 1)
        d = rng.normal(size=(n, 3))
        o[:32], d[:32] = through((-1.0, 1.0, 6.0), (0.0, 2.0, 7.0), 1.5, 32)            # sphere, then sphere
    return o.astype(f32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


@pytest.mark.parametrize("acc", [3, NAIVE])
def test_entry_0_is_the_closest_hit_query(room, acc):
    got, cast = room[acc]
    assert np.array_equal(got["kind"][:, 0], cast[0]) and np.array_equal(got["index"][:, 0], cast[1])
    assert np.array_equal(bits(got["t"][:, 0]), bits(cast[2]))
    assert np.array_equal(got["count"] == 0, cast[0] == 0)
    frac = float((cast[0] > 0).mean())
    assert 0.2 < frac < 0.99 and (cast[0] == LIGHT).sum() >= 16 and (got["count"] >= 2).sum() >= 128
    # the whole lists: the visit set's triangles (BVH) or every triangle (Naive), and the lights
    want = room["scene"].lists(room["o"], room["d"], 8, naive=acc == NAIVE)
    assert_lists(got, want, "room, accelerator %d" % acc)


@pytest.mark.parametrize("scene,kinds", [(3, (PLANE, SPHERE)), (2, (PLANE, SPHERE, LIGHT))])
def test_planes_spheres_and_lights_down_the_list(scene, kinds):
    """Naive tests every primitive: the lists are the float32 restatements of leafPlanes / leafSpheres
    and the kernels' triTest, sorted.  Entry 0 is the closest-hit query under both accelerators."""
    import mobileraytracer_amd as m
    o, d = builtin_rays(scene)
    cfg = m.Config(width=16, height=16, shader=1, sceneIndex=scene, accelerator=NAIVE)
    want = Scene(cfg).lists(o, d, 16, naive=True)
    for k in kinds:  # (on the CPU: every kind occurs behind a first hit)
        assert (want["kind"][:, 1:] == k).sum() >= 4, "too few entries of kind %d down the lists" % k
    with m.Renderer(cfg) as r:
        got = multi(r, o, d, 16)
        cast = tuple(x.cpu().numpy() for x in r.cast_rays(dev(o), dev(d)))
    assert_lists(got, want, "scene %d, Naive" % scene)
    assert np.array_equal(got["kind"][:, 0], cast[0]) and np.array_equal(got["index"][:, 0], cast[1])
    assert np.array_equal(bits(got["t"][:, 0]), bits(cast[2]))
    with m.Renderer(dataclasses.replace(cfg, accelerator=m.ACC_BVH)) as r:
        bvh = multi(r, o, d, 16)
        cast = tuple(x.cpu().numpy() for x in r.cast_rays(dev(o), dev(d)))
    assert np.array_equal(bvh["kind"][:, 0], cast[0]) and np.array_equal(bvh["index"][:, 0], cast[1])
    assert np.array_equal(bits(bvh["t"][:, 0]), bits(cast[2]))
    # BVH against Naive where every plane is crossed well inside its box (the reference boxes a plane as
    # its point +- 100 / sqrt(2) along two axes, Plane.cpp:79-96: a crossing further out is in Naive's
    # hit set and not in the BVH's).  No list is full here: every crossing is listed.
    assert want["count"].max() < 16
    near = ~((want["kind"] == PLANE) & (want["t"] > 40)).any(1)
    assert near.sum() >= 192
    assert_bvh_equals_naive({f: x[near] for f, x in bvh.items()}, {f: x[near] for f, x in got.items()})


# ---- 4. BVH against Naive ----------------------------------------------------------------------------
def assert_bvh_equals_naive(a, b):
    """count, kind and t equal everywhere; index equal outside groups of bit-equal t, inside which the
    two documented orders may differ: there the groups are compared as sets.  (A group cut off by the
    end of a full list is compared up to the kinds: the two orders may keep different members.)"""
    assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["kind"], b["kind"])
    assert np.array_equal(bits(a["t"]), bits(b["t"]))
    K = a["kind"].shape[1]
    tb = bits(a["t"])
    groups = 0
    for i in np.nonzero((a["index"] != b["index"]).any(1))[0]:
        k = 0
        while k < min(a["count"][i], K):
            e = k + 1
            while e < min(a["count"][i], K) and tb[i, e] == tb[i, k]:
                e += 1
            cut = e == K and a["count"][i] > K
            ga = sorted(zip(a["kind"][i, k:e], a["index"][i, k:e]))
            gb = sorted(zip(b["kind"][i, k:e], b["index"][i, k:e]))
            if e - k == 1 or not cut:
                assert ga == gb, (i, k, e, ga, gb)
            groups += e - k > 1
            k = e
    return groups


def test_bvh_and_naive_agree(room):
    """Same rays, same scene, two accelerators.  Compared on every ray whose direction has no zero
    component: a ray with an infinite 1/d that starts on a box plane gets a NaN out of the reference
    slab test, which then fails, so the BVH's visit set (the reference's) lacks leaves whose triangles
    Naive tests - there the two hit sets differ by definition (test_entry_0_... pins each of them)."""
    import mobileraytracer_amd as m
    ok = ~(room["d"] == 0).any(1)
    assert ok.sum() >= 2048 and (~ok).sum() >= 512
    assert_bvh_equals_naive({f: x[ok] for f, x in room[m.ACC_BVH][0].items()}, {f: x[ok] for f, x in room[NAIVE][0].items()})


# ---- 5. the interval and sources ---------------------------------------------------------------------
def test_interval_and_sources(layers):
    import mobileraytracer_amd as m
    sc, _, _, _ = layers(3)
    o = np.array([(0.25, 0.5, 0.0)] * 70, f32)
    d = np.array([(0.0, 0.0, 1.0)] * 70, f32)
    two, above = f32(2.0), np.nextafter(f32(2.0), f32(3.0))
    dist = np.where(np.arange(70) % 2 == 0, two, above).astype(f32)
    with m.Renderer(sc.cfg) as r:
        free = multi(r, o, d, 8)
        assert free["count"].tolist() == [4] * 70 and free["t"][0, :4].tolist() == [1.0, 2.0, 3.0, 4.0]
        got = multi(r, o, d, 8, dist=dist)
        assert_lists(got, sc.lists(o, d, 8, tmax=dist), "dist")
        # t >= dist is absent, t just below it present; the padding holds the ray's own dist
        assert got["count"].tolist() == [1, 2] * 35
        assert (bits(got["t"][0::2, 1:]) == bits(two)).all() and (bits(got["t"][1::2, 2:]) == bits(above)).all()
        assert (got["t"][1::2, 1] == 2.0).all() and (got["kind"][1::2, 1] == TRIANGLE).all()
        # a source triangle removes exactly its own entry
        j = int(free["index"][0, 1])  # the triangle of layer 2 this ray crosses
        src = np.tile(np.array([(TRIANGLE, j)], np.int32), (70, 1))
        got = multi(r, o, d, 8, src=src)
        assert_lists(got, sc.lists(o, d, 8, src=src), "src")
        assert got["count"].tolist() == [3] * 70 and got["t"][0, :3].tolist() == [1.0, 3.0, 4.0]
        assert not (got["index"][:, :3] == j)[got["kind"][:, :3] == TRIANGLE].any()
        # a sphere or light source, a kind that is none, an index out of range: nothing changes
        for pair in ((SPHERE, 0), (LIGHT, 0), (LIGHT, 1), (TRIANGLE, 1 << 20), (TRIANGLE, -1), (7, 0), (0, 0)):
            got = multi(r, o, d, 8, src=np.tile(np.array([pair], np.int32), (70, 1)))
            assert_lists(got, free, "src %s" % (pair,))


# ---- 6. chunks and strides ---------------------------------------------------------------------------
def test_chunks_and_strides(layers):
    import mobileraytracer_amd as m
    sc, _, _, _ = layers(3)
    with m.Renderer(sc.cfg) as r:
        cap = r.queue_info()["rayCap"][0]
        assert cap >= 64
        n = cap + 65
        rng = np.random.default_rng(66)
        rays = np.concatenate([rng.uniform(-0.25, 1.25, (n, 2)), rng.uniform(-1, 5, (n, 1)),
                               rng.normal(size=(n, 2)) * 0.25, rng.choice([-1.0, 1.0], (n, 1))], 1).astype(f32)
        both = dev(rays)
        got = r.cast_multi_hits(both[:, :3], both[:, 3:], 4)  # read in place: rows 6 floats apart
        got = {f: x.cpu().numpy() for f, x in got.items()}
        half = n // 2
        assert half <= cap
        parts = [multi(r, rays[a:b, :3], rays[a:b, 3:], 4) for a, b in ((0, half), (half, n))]
        assert r.queue_info()["rayCap"][0] == cap
    want = {f: np.concatenate([p[f] for p in parts]) for f in FIELDS}
    assert_lists(got, want, "chunks")
    assert (want["count"] > 0).mean() > 0.2 and (want["count"] == 0).sum() >= 16


# ---- 7. deep trees -----------------------------------------------------------------------------------
def test_deep_stack_spills_and_lists_the_lowest_walk_order_copies(tmp_path):
    import mobileraytracer_amd as m
    files = S.write_stack(str(tmp_path), S.STACK_DEEP)
    first = files[3]
    sc = Scene(obj_cfg(files[:3]))
    assert m.walk_stack(sc.cfg)["need"] == S.STACK_CASES[S.STACK_DEEP][1]  # 446: far beyond the LDS stack
    o = np.array([(0.125, 0.125, -9.0), (0.5, -1.0, -9.0), (-0.875, -1.625, -9.0), (4.0, 4.0, -9.0), (0.375, 0.875, -9.0)] * 14, f32)[:67]
    d = np.tile(np.array([(0.0, 0.0, 1.0)], f32), (len(o), 1))
    want = sc.lists(o, d, 16)
    with m.Renderer(sc.cfg) as r:
        got = multi(r, o, d, 16)
    assert_lists(got, want, "stack 450")
    through = np.abs(o[:, 0]) < 3
    copies = first + np.arange(S.STACK_DEEP)
    by_walk = copies[np.argsort(sc.pos[copies])]
    assert (got["count"][through] >= S.STACK_DEEP).all() and (got["count"][~through] < S.STACK_DEEP).all()
    assert (got["index"][through] == by_walk[:16]).all() and (bits(got["t"][through]) == bits(f32(7.0))).all()


# ---- 8. wanted outputs only --------------------------------------------------------------------------
def test_only_the_wanted_outputs_are_written(layers):
    import torch
    import mobileraytracer_amd as m
    sc, o, d, want16 = layers(3)
    n, K, guard = len(o), 4, 64
    want = prefix(want16, K)
    widths = {"count": 1, "kind": K, "index": K, "t": K, "bary": 2 * K}

    def outputs():
        return {f: torch.full((guard + n * w + guard,), SENTINEL, dtype=torch.int32, device="cuda") for f, w in widths.items()}

    do, dd = dev(o), dev(d)
    with m.Renderer(sc.cfg) as r:
        for wanted in (("count",), ("t",), FIELDS):
            out = outputs()
            torch.cuda.synchronize()  # (stream 0 is the renderer's own stream: not ordered after torch's fills)
            r.cast_multi_hits_device(do.data_ptr(), dd.data_ptr(), n, K,
                                     **{"d_" + f: out[f][guard:].data_ptr() for f in wanted})
            torch.cuda.synchronize()
            for f, w in widths.items():
                x = out[f].cpu().numpy()
                assert (x[:guard] == SENTINEL).all() and (x[guard + n * w:] == SENTINEL).all(), (wanted, f)
                body = x[guard:guard + n * w]
                if f in wanted:
                    e = want[f] if want[f].dtype == np.int32 else bits(want[f])
                    assert np.array_equal(body, e.reshape(-1)), (wanted, f)
                else:
                    assert (body == SENTINEL).all(), (wanted, f)


# ---- 9. state ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """shape_scenes' lit base (a frame of it is no single colour), 70 rays in from its camera's side and
    their expected lists at K = 16."""
    sc = Scene(obj_cfg(S.write_base(str(tmp_path_factory.mktemp("multi_base")))))
    rng = np.random.default_rng(99)
    o = np.stack([rng.uniform(-4, 4, 70), rng.uniform(-4, 4, 70), np.full(70, -9.0)], 1).astype(f32)
    d = np.stack([rng.uniform(-0.25, 0.25, 70), rng.uniform(-0.25, 0.25, 70), np.ones(70)], 1).astype(f32)
    return sc, o, d, sc.lists(o, d, 16)


def test_a_query_leaves_the_frames_and_totals_alone(base):
    import mobileraytracer_amd as m
    sc, o, d, want16 = base
    assert (want16["count"] >= 2).sum() >= 16
    cfg = dataclasses.replace(sc.cfg, width=32, height=32)

    def frame(r):
        bm = np.zeros(32 * 32, np.int32)
        r.render_frame(bm)
        return bm, r.frame_rays()

    with m.Renderer(cfg) as plain:
        ref = [frame(plain), frame(plain)]
        ref_total = plain.get_total_casted_rays()
    with m.Renderer(cfg) as r:
        a = frame(r)
        total = r.get_total_casted_rays()
        got = multi(r, o, d, 16)
        assert r.get_total_casted_rays() == total
        b = frame(r)
        assert r.get_total_casted_rays() == ref_total
    assert_lists(got, want16, "between two frames")
    assert np.array_equal(a[0], ref[0][0]) and a[1] == ref[0][1]
    assert np.array_equal(b[0], ref[1][0]) and b[1] == ref[1][1]
    assert a[1][0] > 0 and len(set(a[0].tolist())) > 1


# ---- 10. refusals ------------------------------------------------------------------------------------
def test_regular_grid_and_device_groups_are_refused(base):
    import torch
    import mobileraytracer_amd as m
    sc, o, d, _ = base
    do, dd = dev(o), dev(d)
    count = torch.full((len(o),), SENTINEL, dtype=torch.int32, device="cuda")
    for cfg, message in ((dataclasses.replace(sc.cfg, accelerator=GRID), "RegularGrid"),
                         (m.Config(width=16, height=16, shader=1, sceneIndex=0, devices=[0, 0]), "device groups are not supported")):
        with m.Renderer(cfg) as r:
            before = np.zeros(16 * 16, np.int32)
            r.render_frame(before)
            total = r.get_total_casted_rays()
            with pytest.raises(RuntimeError, match=message):
                r.cast_multi_hits_device(do.data_ptr(), dd.data_ptr(), len(o), 4, d_count=count.data_ptr())
            with pytest.raises(RuntimeError, match=message):
                r.cast_multi_hits(do, dd, 4)
            torch.cuda.synchronize()
            assert (count.cpu().numpy() == SENTINEL).all() and r.get_total_casted_rays() == total
            after = np.zeros(16 * 16, np.int32)
            r.render_frame(after)
            assert np.array_equal(before, after) and len(set(before.tolist())) > 1


# ---- 11. non-finite geometry -------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 16])
def test_non_finite_geometry_keeps_the_lists_ordered(tmp_path, K):
    import mobileraytracer_amd as m
    files = S.write_inf_vertex(str(tmp_path))
    cfg = obj_cfg(files[:3])
    rng = np.random.default_rng(111)
    n = 1025
    # from inside the room, half of them downward past the floor: those reach the non-finite leaf
    o = np.stack([rng.uniform(-7, 7, n), rng.uniform(-4, 4, n), rng.uniform(-9, 1.5, n)], 1).astype(f32)
    d = rng.normal(size=(n, 3))
    d[::2, 1] = -np.abs(d[::2, 1]) - 0.5
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    dist = np.where(np.arange(n) % 3 == 0, rng.uniform(1, 30, n), RAY_MAX).astype(f32)
    with m.Renderer(cfg) as r:
        got = multi(r, o, d, K, dist=dist)  # (returns 0: no exception)
    listed = np.minimum(got["count"], K)
    assert (got["count"] >= 0).all() and (got["count"] > 0).mean() > 0.3
    for i in range(n):
        t = got["t"][i, :listed[i]]
        assert not np.isnan(t).any() and (t >= EPS).all() and (t < dist[i]).all()
        assert (np.diff(t) >= 0).all()
        assert (got["kind"][i, :listed[i]] > 0).all() and (got["kind"][i, listed[i]:] == 0).all()
        assert (bits(got["t"][i, listed[i]:]) == bits(dist[i])).all()


# ---- the wrapper -------------------------------------------------------------------------------------
def test_wrapper_handles_empty_batches_bad_k_and_bad_fields(layers):
    import torch
    import mobileraytracer_amd as m
    sc, o, d, _ = layers(1)
    do, dd = dev(o), dev(d)
    with m.Renderer(sc.cfg) as r:
        empty = r.cast_multi_hits(do[:0], dd[:0], 4)
        assert set(empty) == set(FIELDS) and empty["count"].shape == (0,) and empty["bary"].shape == (0, 4, 2)
        assert empty["kind"].dtype == torch.int32 and empty["t"].dtype == torch.float32
        only = r.cast_multi_hits(do, dd, 2, fields=("count", "t"))
        assert set(only) == {"count", "t"} and only["t"].shape == (len(o), 2)
        for k in (0, 17):
            with pytest.raises(ValueError):
                r.cast_multi_hits(do, dd, k)
            with pytest.raises(RuntimeError, match="K must be"):
                r.cast_multi_hits_device(do.data_ptr(), dd.data_ptr(), len(o), k, d_count=only["count"].data_ptr())
        with pytest.raises(ValueError):
            r.cast_multi_hits(do, dd, 4, fields=("depth",))
        with pytest.raises(ValueError):
            r.cast_multi_hits(do, dd, 4, fields=())
