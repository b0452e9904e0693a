"""Nearest-point queries (mrt_nearest_points_device): which primitive is nearest to each point, the squared
distance, the point on it and its barycentrics.  Every comparison is exact (kind, index, and the bits of
dist2, point and bary) against answers built on the host: mrt_point_distance on every candidate of the
scene accessors, the documented total order applied in NumPy (nearest_cases.Candidates).  `tests` is
diagnostic and compared nowhere, only bounded where the cull is the subject.

Frames are 16 x 16; outputs given to the C entry point start filled with a sentinel."""
import dataclasses
import os

import numpy as np
import pytest

import nearest_cases as N
import shape_scenes as S
from test_cast_rays_gpu import SENTINEL, bits, dev, water_cfg

pytestmark = pytest.mark.gpu

f32 = np.float32
NAIVE, GRID, BVH = 1, 2, 3
WIDTHS = {"kind": 1, "index": 1, "dist2": 1, "point": 3, "bary": 2, "tests": 1}
ALL = tuple(WIDTHS)


def nearest(r, points, max_dist=None, src=None, fields=None):
    got = r.nearest_points(dev(points), max_dist=None if max_dist is None else dev(max_dist),
                           src=None if src is None else dev(src), fields=fields)
    return {f: x.cpu().numpy() for f, x in got.items()}


def obj_cfg(files, **kw):
    import mobileraytracer_amd as m
    return m.Config(width=16, height=16, shader=1, sceneIndex=-1, objFilePath=files[0], mtlFilePath=files[1],
                    camFilePath=files[2], **kw)


def both(cfg, points, want, what, **kw):
    """The query under BVH and Naive: each equals the host's answer, so they equal each other bit for bit."""
    import mobileraytracer_amd as m
    out = {}
    for acc in (BVH, NAIVE):
        with m.Renderer(dataclasses.replace(cfg, accelerator=acc)) as r:
            out[acc] = nearest(r, points, **kw)
        N.assert_same(out[acc], want, "%s, accelerator %d" % (what, acc))
    N.assert_same(out[BVH], out[NAIVE], what + ", BVH against Naive")
    return out


# ---- scenes the tests write --------------------------------------------------------------------------
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


def soup(path, name, offset, size, seed):
    """300 random triangles of about `size` with their centres in the unit cube at `offset`, and an
    emissive quad above it (two area lights)."""
    rng = np.random.default_rng(seed)
    c = offset + rng.random((300, 1, 3))
    v = (c + size * rng.normal(size=(300, 3, 3))).astype(f32)
    lo, hi = f32(offset - 0.5), f32(offset + 1.5)
    light = [(lo, hi, lo), (hi, hi, lo), (hi, hi, hi), (lo, hi, hi)]
    return write_mesh(path, name, tris=[tuple(map(tuple, t)) for t in v], light=light)


FAR_LIGHT = [(0, 0, 64), (1, 0, 64), (1, 1, 64), (0, 1, 64)]  # (a scene needs a light; this one is never the nearest)


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


# ---- 1. known answers --------------------------------------------------------------------------------
def test_device_functions_equal_the_hosts_bit_for_bit():
    import mobileraytracer_amd as m
    tri, p = N.random_pairs(4096, 21)
    dtri, dp = N.degenerate_triangles()
    ex = N.exact_triangle()
    rng = np.random.default_rng(22)
    planes = rng.normal(size=(2048, 6))
    planes[:, :3] /= np.linalg.norm(planes[:, :3], axis=1, keepdims=True)
    spheres = np.concatenate([rng.normal(size=(2048, 3)) * 4, rng.uniform(0.01, 9, (2048, 1))], 1)
    sp = spheres[:, :3] + rng.normal(size=(2048, 3)) * rng.choice([0.0, 1.0, 10.0], (2048, 1))  # (a third at the centre)
    cases = [(N.TRIANGLE, np.concatenate([tri, dtri, ex[0]]), np.concatenate([p, dp, ex[1]])),
             (N.LIGHT, tri[:1024], p[:1024]),
             (N.PLANE, np.concatenate([planes.astype(f32), N.exact_plane()[0]]),
              np.concatenate([(rng.normal(size=(2048, 3)) * 10).astype(f32), N.exact_plane()[1]])),
             (N.SPHERE, np.concatenate([spheres.astype(f32), N.exact_sphere()[0]]),
              np.concatenate([sp.astype(f32), N.exact_sphere()[1]]))]
    for kind, prims, pts in cases:
        host = m.point_distance(kind, prims, pts)
        got = m.kat_point_distance(kind, prims, pts)
        for name, h, g in zip(("dist2", "nearest", "bary"), host, got):
            bad = (bits(h) != bits(g)).reshape(len(pts), -1).any(1)
            assert not bad.any(), "kind %d %s: %d of %d pairs differ, first %d: host %s device %s" % (
                kind, name, bad.sum(), len(pts), np.argmax(bad), h[np.argmax(bad)], g[np.argmax(bad)])


# ---- 2. a soup ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,size,near", [(0.0, 0.2, 1e-3), (1024.0, 0.01, 1e-4)])
def test_soup_under_both_accelerators(tmp_path, offset, size, near):
    import mobileraytracer_amd as m
    cfg = obj_cfg(soup(str(tmp_path), "soup", offset, size, 31))
    geom = m.scene_triangles(cfg)[0]
    assert len(geom) == 300
    rng = np.random.default_rng(32)
    corners = np.concatenate([geom[:, 0], geom[:, 0] + geom[:, 1], geom[:, 0] + geom[:, 2]])
    lo, hi = corners.min(0).astype(np.float64), corners.max(0).astype(np.float64)
    k = 667
    pts = np.concatenate([rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (k, 3)),  # a box twice the scene's
                          surface_points(geom, k, rng, near), corner_points(geom, k - 1, rng)]).astype(f32)
    assert len(pts) == 2000
    want = N.Candidates(cfg).expected(pts)
    assert (want["kind"] == N.TRIANGLE).mean() > 0.75 and (want["dist2"] == 0).sum() >= 100
    both(cfg, pts, want, "soup at %g" % offset)


# ---- 3. exact ties -----------------------------------------------------------------------------------
def test_exact_ties_go_to_the_lowest_input_index(tmp_path):
    import mobileraytracer_amd as m
    cfg = obj_cfg(write_mesh(str(tmp_path), "sheets", quads=sheet_quads(16, 0) + sheet_quads(16, 2), light=FAR_LIGHT))
    geom = m.scene_triangles(cfg)[0]
    assert len(geom) == 1024
    corners = np.concatenate([geom[:, 0], geom[:, 0] + geom[:, 1], geom[:, 0] + geom[:, 2]])
    lo = corners.min(0)
    assert (corners.max(0) - lo).tolist() == [16.0, 16.0, 2.0]
    g = np.arange(33, dtype=f32) * f32(0.5)  # corners, edge midpoints and cell centres
    pts = np.stack([lo[0] + np.repeat(g, 33), lo[1] + np.tile(g, 33), np.full(33 * 33, lo[2] + 1, f32)], 1).astype(f32)
    cands = N.Candidates(cfg)
    want = cands.expected(pts)
    # (on the host: every point is one unit from both sheets, and several triangles tie for most)
    assert (want["dist2"] == 1.0).all() and (want["kind"] == N.TRIANGLE).all()
    d2 = m.point_distance(N.TRIANGLE, np.tile(geom.reshape(-1, 9), (len(pts), 1)), np.repeat(pts, 1024, 0))[0].reshape(-1, 1024)
    ties = (d2 == 1.0).sum(1)
    assert (ties >= 2).all() and (ties >= 4).sum() >= 256
    assert np.array_equal(want["index"], (d2 == 1.0).argmax(1))  # the lowest input index among them
    both(cfg, pts, want, "two sheets")


# ---- 4. the cull -------------------------------------------------------------------------------------
def test_the_cull_skips_most_of_a_sheet(tmp_path):
    import mobileraytracer_amd as m
    cfg = obj_cfg(write_mesh(str(tmp_path), "sheet46", quads=sheet_quads(46, 0), light=FAR_LIGHT))
    geom = m.scene_triangles(cfg)[0]
    T = len(geom)
    assert T == 4232
    corners = np.concatenate([geom[:, 0], geom[:, 0] + geom[:, 1], geom[:, 0] + geom[:, 2]])
    lo = corners.min(0)
    rng = np.random.default_rng(41)
    pts = np.concatenate([lo[:2] + rng.integers(0, 46, (1024, 2)) + rng.random((1024, 2)), np.full((1024, 1), lo[2] + 0.5)], 1).astype(f32)
    want = N.Candidates(cfg).expected(pts)
    got = both(cfg, pts, want, "sheet")
    assert (got[NAIVE]["tests"] == T + 2).all()  # Naive: every triangle and the two area lights
    got = got[BVH]
    mean = got["tests"].mean()
    print("46 x 46 sheet: %d triangles, mean tests per point %.1f (a walk that never culls: %d)" % (T, mean, T))
    assert (got["tests"] >= 1).all() and mean < T / 8


# ---- 5. tree shapes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack%d" % S.STACK_DEEP, "degenerate", "inf_vertex", "outlier"])
def test_tree_shapes(tmp_path, name):
    import mobileraytracer_amd as m
    files = S.write_scene(str(tmp_path), name)
    cfg = obj_cfg(files[:3])
    if name.startswith("stack"):
        assert m.walk_stack(cfg)["need"] == S.STACK_CASES[S.STACK_DEEP][1]  # far beyond the LDS stack
    rng = np.random.default_rng(51)
    geom = m.scene_triangles(cfg)[0]
    pts = np.concatenate([rng.uniform((-9, -13, -11), (9, 10, 41), (128, 3)), surface_points(geom, 64, rng, 1e-3),
                          corner_points(geom, 64, rng)]).astype(f32)
    pts = pts[np.isfinite(pts).all(1)]
    assert len(pts) >= 192
    want = N.Candidates(cfg).expected(pts)
    assert not np.isnan(want["dist2"]).any() and (want["kind"] > 0).all()
    got = both(cfg, pts, want, name)
    assert not np.isnan(got[BVH]["dist2"]).any()


# ---- 6. the other kinds ------------------------------------------------------------------------------
def builtin_points(cfg, n, seed):
    """Uniform points in a box about the scene's finite primitives, and points near each kind's surfaces
    (found with mrt_point_distance's nearest point: no geometry is restated)."""
    import mobileraytracer_amd as m
    rng = np.random.default_rng(seed)
    cands = N.Candidates(cfg)
    rec = {k: r[c] for k, r, c in cands.sets}
    anchors = [rec[N.SPHERE][:, :3]] if len(rec[N.SPHERE]) else []
    for k in (N.TRIANGLE, N.LIGHT):
        if len(rec[k]):
            anchors += [rec[k][:, :3], rec[k][:, :3] + rec[k][:, 3:6], rec[k][:, :3] + rec[k][:, 6:]]
    a = np.concatenate(anchors).astype(np.float64)
    lo, hi = a.min(0) - 1, a.max(0) + 1
    parts = [rng.uniform(lo, hi, (n // 2, 3)).astype(f32)]
    kinds = [k for k in (N.PLANE, N.SPHERE, N.TRIANGLE, N.LIGHT) if len(rec[k])]
    per = (n - n // 2) // len(kinds)
    for k in kinds:
        seeds = rng.uniform(lo, hi, (per, 3)).astype(f32)
        q = m.point_distance(k, rec[k][rng.integers(0, len(rec[k]), per)], seeds)[1]
        parts.append((q + rng.uniform(-1e-3, 1e-3, (per, 3))).astype(f32))
    pts = np.concatenate(parts)
    return cands, np.concatenate([pts, rng.uniform(lo, hi, (n - len(pts), 3)).astype(f32)])


def test_planes_spheres_triangles_and_lights():
    import mobileraytracer_amd as m
    seen = set()
    for scene in (2, 3):
        cfg = m.Config(width=16, height=16, shader=1, sceneIndex=scene)
        cands, pts = builtin_points(cfg, 1024, 60 + scene)
        want = cands.expected(pts)
        kinds = {k: int((want["kind"] == k).sum()) for k in (1, 2, 3, 4)}
        print("scene %d: candidates %s, answers per kind %s" % (scene, cands.count, kinds))
        for k, count in cands.count.items():  # (on the host: every kind the scene holds answers some points)
            assert kinds[k] >= 8 or count == 0 or (k == N.LIGHT and not cands.sets[-1][2].any()), (scene, k)
        seen |= {k for k, c in kinds.items() if c >= 8}
        both(cfg, pts, want, "scene %d" % scene)
        # an accelerator id that builds nothing: the area lights only
        lights = N.Candidates(cfg, lights_only=True)
        want0 = lights.expected(pts)
        assert set(np.unique(want0["kind"])) <= {0, N.LIGHT}
        with m.Renderer(dataclasses.replace(cfg, accelerator=0)) as r:
            N.assert_same(nearest(r, pts), want0, "scene %d, no accelerator" % scene)
        if lights.sets[-1][2].any():
            assert (want0["kind"] == N.LIGHT).all()
    assert seen == {1, 2, 3, 4}


# ---- 7. radius and sources ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """shape_scenes' lit base (a frame of it is no single colour), 1030 points in and about its room and
    the host's answers."""
    import mobileraytracer_amd as m
    cfg = obj_cfg(S.write_base(str(tmp_path_factory.mktemp("nearest_base"))))
    rng = np.random.default_rng(71)
    geom = m.scene_triangles(cfg)[0]
    pts = np.concatenate([rng.uniform((-9, -6, -11), (9, 10, 4), (518, 3)), surface_points(geom, 512, rng, 1e-3)]).astype(f32)
    cands = N.Candidates(cfg)
    b = {"cfg": cfg, "geom": geom, "pts": pts, "cands": cands, "want": cands.expected(pts)}
    pts.setflags(write=False)
    return b


def test_radius(base):
    import mobileraytracer_amd as m
    pts, want = base["pts"], base["want"]
    n = len(pts)
    rng = np.random.default_rng(72)
    d = np.sqrt(want["dist2"].astype(np.float64))
    radius = (d * rng.choice([0.5, 0.999, 1.001, 2.0], n)).astype(f32)
    radius[d == 0] = f32(0.25)
    special = np.array([0.0, -1.0, np.nan, -np.inf, -0.0], f32)
    radius[:len(special) * 6] = np.tile(special, 6)
    want_r = base["cands"].expected(pts, max_dist=radius)
    missed = want_r["kind"] == 0
    assert 0.2 < missed.mean() < 0.8 and missed[:len(special) * 6].all()
    # the miss record: every field as defined
    assert (want_r["index"][missed] == -1).all() and (want_r["point"][missed] == 0).all() and (want_r["bary"][missed] == 0).all()
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(want_r["dist2"][missed]), bits(np.where(radius > 0, radius * radius, f32(0)).astype(f32)[missed]))
    # a found answer is the unbounded one
    N.assert_same({f: x[~missed] for f, x in want_r.items()}, {f: x[~missed] for f, x in want.items()}, "found")
    both(base["cfg"], pts, want_r, "radius", max_dist=radius)


def test_sources(base):
    import mobileraytracer_amd as m
    geom, cfg = base["geom"], base["cfg"]
    rng = np.random.default_rng(73)
    n = 515
    j = rng.integers(0, len(geom), n)
    w = np.array([(0.25, 0.25), (0.5, 0.25), (0.125, 0.5)], f32)[rng.integers(0, 3, n)]
    t = geom.reshape(-1, 9)[j]
    pts = ((t[:, :3] + t[:, 3:6] * w[:, :1]) + t[:, 6:] * w[:, 1:]).astype(f32)  # exactly on triangle j (dyadic coordinates)
    free = base["cands"].expected(pts)
    assert (free["dist2"] == 0).all()
    src = np.stack([np.full(n, N.TRIANGLE), j], 1).astype(np.int32)
    want = base["cands"].expected(pts, src=src)
    assert not ((want["kind"] == N.TRIANGLE) & (want["index"] == j)).any() and (want["kind"] > 0).all()
    assert (want["dist2"] > 0).mean() > 0.5
    got = both(cfg, pts, want, "sources", src=src)
    assert not ((got[BVH]["kind"] == N.TRIANGLE) & (got[BVH]["index"] == j)).any()
    # a sphere or light source, a kind that is none, an index out of range: no source
    with m.Renderer(cfg) as r:
        for pair in ((N.SPHERE, 0), (N.LIGHT, 0), (N.LIGHT, 1), (N.TRIANGLE, 1 << 20), (N.TRIANGLE, -1), (N.PLANE, 0), (7, 0), (0, 0)):
            got = nearest(r, pts, src=np.tile(np.array([pair], np.int32), (n, 1)))
            N.assert_same(got, free, "src %s" % (pair,))


# ---- 8. chunks and layout ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def water():
    """tests/golden/CornellBox (Water) at 16 x 16: a small level-1 queue; n = 3 cap + 65 points in a box
    about the scene and the host's answers."""
    import mobileraytracer_amd as m
    cfg = water_cfg()
    with m.Renderer(cfg) as r:
        cap = r.queue_info()["rayCap"][0]
    assert cap >= 64
    boxes, _, _, _ = m.triangle_bvh(cfg)
    lo, hi = boxes[0, :3].astype(np.float64), boxes[0, 3:].astype(np.float64)
    n = 3 * cap + 65
    pts = np.random.default_rng(81).uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), (n, 3)).astype(f32)
    want = N.Candidates(cfg).expected(pts)
    assert (want["kind"] > 0).all() and len(np.unique(want["index"])) > 100
    pts.setflags(write=False)
    return {"cfg": cfg, "cap": cap, "pts": pts, "want": want}


def test_chunks_and_a_stride_of_six(water):
    import mobileraytracer_amd as m
    pts = water["pts"]
    wide = np.concatenate([pts, np.full((len(pts), 3), 7.0, f32)], 1)
    with m.Renderer(water["cfg"]) as r:
        got = nearest(r, pts)
        rows = dev(wide)
        strided = {f: x.cpu().numpy() for f, x in r.nearest_points(rows[:, :3]).items()}  # read in place: rows 6 floats apart
        assert r.queue_info()["rayCap"][0] == water["cap"]  # the chunking assumed
    N.assert_same(got, water["want"], "3 cap + 65 points")
    N.assert_same(strided, water["want"], "stride 6")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches_and_single_fields_write_their_entries_and_nothing_else(water, n):
    import ctypes
    import torch
    import mobileraytracer_amd as m
    guard = 64
    want = {f: x[:n] for f, x in water["want"].items()}
    dp = dev(water["pts"][:n])

    def outputs():
        return {f: torch.full((guard + n * w + guard,), SENTINEL, dtype=torch.int32, device="cuda") for f, w in WIDTHS.items()}

    def check(out, wanted, what):
        res = {}
        for f, w in WIDTHS.items():
            x = out[f].cpu().numpy()
            assert (x[:guard] == SENTINEL).all() and (x[guard + n * w:] == SENTINEL).all(), (what, f)
            body = x[guard:guard + n * w]
            if f not in wanted:
                assert (body == SENTINEL).all(), (what, f)
            elif f != "tests":
                e = want[f] if want[f].dtype == np.int32 else bits(want[f])
                assert np.array_equal(body, e.reshape(-1)), (what, f)
            res[f] = body
        return res

    with m.Renderer(water["cfg"]) as r:
        runs = [ALL] + [(f,) for f in ALL]
        tests_all = None
        for wanted in runs:
            out = outputs()
            torch.cuda.synchronize()  # (stream 0 is the renderer's own stream: not ordered after torch's fills)
            r.nearest_points_device(dp.data_ptr(), n, **{"d_" + f: out[f][guard:].data_ptr() for f in wanted})
            torch.cuda.synchronize()
            res = check(out, wanted, wanted)
            if wanted == ALL:
                tests_all = res["tests"]
                assert (tests_all >= 1).all()
            elif wanted == ("tests",):
                assert np.array_equal(res["tests"], tests_all)
        # a smaller outSize: the cut-off fields count as NULL
        out = outputs()
        torch.cuda.synchronize()
        r.nearest_points_device(dp.data_ptr(), n, out_size=3 * ctypes.sizeof(ctypes.c_void_p),
                                **{"d_" + f: out[f][guard:].data_ptr() for f in ALL})
        torch.cuda.synchronize()
        check(out, ("kind", "index", "dist2"), "outSize 24")


# ---- 9. state ----------------------------------------------------------------------------------------
def test_a_query_leaves_frames_totals_and_ray_queries_alone(base):
    import mobileraytracer_amd as m
    cfg = dataclasses.replace(base["cfg"], width=32, height=32)
    pts, want = base["pts"], base["want"]
    rng = np.random.default_rng(91)
    o = np.stack([rng.uniform(-4, 4, 200), rng.uniform(-4, 4, 200), np.full(200, -9.0)], 1).astype(f32)
    d = np.stack([rng.uniform(-0.25, 0.25, 200), rng.uniform(-0.25, 0.25, 200), np.ones(200)], 1).astype(f32)

    def frame(r):
        bm = np.zeros(32 * 32, np.int32)
        r.render_frame(bm)
        st = r.frame_stats()
        return bm, r.frame_rays(), {k: v for k, v in st.items() if not k.endswith("Ms")}

    def cast(r):
        return tuple(x.cpu().numpy() for x in r.cast_rays(dev(o), dev(d)))

    with m.Renderer(cfg) as plain:
        ref = [frame(plain), frame(plain)]
        ref_total = plain.get_total_casted_rays()
        ref_cast = cast(plain)
    with m.Renderer(cfg) as r:
        a = frame(r)
        total, stats = r.get_total_casted_rays(), r.frame_stats()
        bytes0 = r.scene_info()["deviceBytes"]
        got = nearest(r, pts)
        bytes1 = r.scene_info()["deviceBytes"]
        n_prims = sum(r.scene_info()[k] for k in ("triangles", "planes", "spheres"))
        assert 0 <= bytes1 - bytes0 <= 4 * n_prims + 4096  # the mapping tables, at the first query only
        before = cast(r)
        again = nearest(r, pts, fields=("kind", "dist2"))
        after = cast(r)
        assert r.scene_info()["deviceBytes"] == bytes1
        assert r.get_total_casted_rays() == total
        now = r.frame_stats()
        assert all(now[k] == stats[k] for k in stats if not k.endswith("Ms"))
        b = frame(r)
        assert r.get_total_casted_rays() == ref_total
    N.assert_same(got, want, "between two frames")
    N.assert_same(again, want, "again", fields=("kind", "dist2"))
    for q in (before, after):
        assert np.array_equal(q[0], ref_cast[0]) and np.array_equal(q[1], ref_cast[1]) and np.array_equal(bits(q[2]), bits(ref_cast[2]))
    assert (ref_cast[0] > 0).mean() > 0.5
    for x, y in ((a, ref[0]), (b, ref[1])):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2]
    assert a[1][0] > 0 and len(set(a[0].tolist())) > 1


def test_query_is_ordered_on_the_callers_stream(water):
    """On a stream of the caller's: a long run of kernels, then the kernel that fills the point tensor, then
    the query, then reductions of its outputs - and no synchronisation before the final copies.  A query
    that started before the fill would answer for the origin, a reduction that started before the query
    would read the sentinel."""
    import torch
    import mobileraytracer_amd as m
    n = len(water["pts"])
    src_p = dev(water["pts"])
    want = [dev(x) for x in (water["want"]["kind"], water["want"]["index"], bits(water["want"]["dist2"]))]
    busy = torch.ones(1 << 24, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with m.Renderer(water["cfg"]) as r:
        with torch.cuda.stream(stream):
            p = torch.zeros(n, 3, device="cuda")
            k = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
            i = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
            t = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
            for _ in range(200):
                busy.mul_(1.0001)
            p.add_(src_p)
            r.nearest_points_device(p.data_ptr(), n, d_kind=k.data_ptr(), d_index=i.data_ptr(), d_dist2=t.data_ptr(),
                                    stream=stream.cuda_stream)
            wrong = (k != want[0]).sum() + (i != want[1]).sum() + (t != want[2]).sum()
            wrong = int(wrong.cpu())  # (the first wait for the device)
    assert wrong == 0


# ---- 10. refusals ------------------------------------------------------------------------------------
def test_regular_grid_and_device_groups_are_refused(base):
    import torch
    import mobileraytracer_amd as m
    dp = dev(base["pts"])
    n = len(base["pts"])
    kind = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    for cfg, message in ((dataclasses.replace(base["cfg"], accelerator=GRID), "RegularGrid"),
                         (m.Config(width=16, height=16, shader=1, sceneIndex=0, devices=[0, 0]), "device groups are not supported")):
        with m.Renderer(cfg) as r:
            total = r.get_total_casted_rays()
            with pytest.raises(RuntimeError, match=message):
                r.nearest_points_device(dp.data_ptr(), n, d_kind=kind.data_ptr())
            with pytest.raises(RuntimeError, match=message):
                r.nearest_points(dp)
            torch.cuda.synchronize()
            assert (kind.cpu().numpy() == SENTINEL).all() and r.get_total_casted_rays() == total


# ---- the wrapper -------------------------------------------------------------------------------------
def test_wrapper_handles_empty_batches_and_bad_fields(base):
    import torch
    import mobileraytracer_amd as m
    dp = dev(base["pts"][:70])
    with m.Renderer(base["cfg"]) as r:
        assert r.NEAREST_FIELDS == ALL
        empty = r.nearest_points(dp[:0])
        assert set(empty) == set(ALL) and empty["kind"].shape == (0,) and empty["point"].shape == (0, 3)
        assert empty["bary"].shape == (0, 2) and empty["kind"].dtype == torch.int32 and empty["dist2"].dtype == torch.float32
        only = r.nearest_points(dp, fields=("dist2", "point"))
        assert set(only) == {"dist2", "point"} and only["point"].shape == (70, 3)
        N.assert_same({f: x.cpu().numpy() for f, x in only.items()}, {f: x[:70] for f, x in base["want"].items()},
                      "two fields", fields=("dist2", "point"))
        for bad in (("depth",), ()):
            with pytest.raises(ValueError):
                r.nearest_points(dp, fields=bad)
        with pytest.raises(TypeError):
            r.nearest_points_device(dp.data_ptr(), 70, d_normal=dp.data_ptr())
