"""Sweep queries (mrt_sweep_spheres_device): the first contact of a sphere moving along each ray - whether,
which primitive, t, the centre there, the contact point and its barycentrics.  Every comparison is exact (ints,
and the bits of t, centre, point and bary) against answers built on the host: mrt_sphere_sweep on every
candidate of the scene accessors, the documented total order applied in NumPy (sweep_cases.Lists).  Every case
runs under BVH and Naive, with all fields and with `hit` only.  `tests` is diagnostic and compared nowhere, only
bounded where the cull is the subject.

Frames are 16 x 16; outputs given to the C entry point start filled with a sentinel."""
import dataclasses

import numpy as np
import pytest

import neighbour_cases as NB
import shape_scenes as S
import sweep_cases as C
from test_cast_rays_gpu import SENTINEL, bits, dev, water_cfg

pytestmark = pytest.mark.gpu

f32 = np.float32
NAIVE, GRID, BVH = 1, 2, 3
ALL = tuple(C.WIDTHS)
INF = f32(np.inf)


def sweep(r, rays, max_t=None, src=None, fields=ALL, stride=None):
    """mrt_sweep_spheres_device on sentinel-filled outputs; rays (n, 7): o, d, r."""
    import torch
    rays = np.ascontiguousarray(rays, f32)
    n = len(rays)
    if stride is None:
        o, d, os_, ds_ = dev(np.ascontiguousarray(rays[:, :3])), dev(np.ascontiguousarray(rays[:, 3:6])), 3, 3
    else:  # origin and direction rows of one (n, stride) array, read in place
        wide = np.full((n, stride), 7.0, f32)
        wide[:, :6] = rays[:, :6]
        rows = dev(wide)
        o, d, os_, ds_ = rows, rows[:, 3:], stride, stride
    rad = dev(np.ascontiguousarray(rays[:, 6]))
    dist = None if max_t is None else dev(np.ascontiguousarray(max_t, f32))
    s = None if src is None else dev(np.ascontiguousarray(src, np.int32))
    out = {f: torch.full((n * C.WIDTHS[f],), SENTINEL, dtype=torch.int32, device="cuda") for f in fields}
    torch.cuda.synchronize()  # (stream 0 is the renderer's own stream: not ordered after torch's fills)
    r.sweep_spheres_device(o.data_ptr(), d.data_ptr(), rad.data_ptr(), n, d_dist=0 if dist is None else dist.data_ptr(),
                           d_src=0 if s is None else s.data_ptr(), orig_stride=os_, dir_stride=ds_,
                           **{"d_" + f: x.data_ptr() for f, x in out.items()})
    torch.cuda.synchronize()
    res = {}
    for f, x in out.items():
        a = x.cpu().numpy()
        if f in ("t", "centre", "point", "bary"):
            a = a.view(f32)
        res[f] = a if C.WIDTHS[f] == 1 else a.reshape(n, C.WIDTHS[f])
    return res


def both(cfg, rays, want, what, accelerators=(BVH, NAIVE), **kw):
    """The query under BVH and Naive, with all fields and with `hit` only: each equals the host's answer, so they
    equal each other bit for bit."""
    import mobileraytracer_amd as m
    out = {}
    for acc in accelerators:
        with m.Renderer(dataclasses.replace(cfg, accelerator=acc)) as r:
            out[acc] = sweep(r, rays, **kw)
            only = sweep(r, rays, fields=("hit", "tests"), **kw)
        C.assert_same(out[acc], want, "%s, accelerator %d" % (what, acc))
        assert not (out[acc]["tests"] == SENTINEL).any()
        assert np.array_equal(only["hit"], want["hit"]), "%s, accelerator %d, hit only" % (what, acc)
        assert (only["tests"] <= out[acc]["tests"]).all()  # (the walk stops at the first acceptance)
        out[acc, "hit"] = only
    if BVH in out and NAIVE in out:
        C.assert_same(out[BVH], out[NAIVE], what + ", BVH against Naive")
    return out


# ---- 1. known answers --------------------------------------------------------------------------------
def test_device_functions_equal_the_hosts_bit_for_bit():
    import mobileraytracer_amd as m
    rng = np.random.default_rng(21)
    for kind, maker in ((C.TRIANGLE, C.triangle_sweeps), (C.LIGHT, C.triangle_sweeps), (C.PLANE, C.plane_sweeps),
                        (C.SPHERE, C.sphere_sweeps)):
        prims, rays = maker(1 << 16, 20 + kind)
        rows = rng.integers(0, len(rays), 4096)  # invalid sweeps: a NaN, an infinity or a negative radius
        rays[rows[:3072], rng.integers(0, 7, 3072)] = rng.choice(np.array([np.nan, np.inf, -np.inf], f32), 3072)
        rays[rows[3072:], 6] = -rays[rows[3072:], 6] - f32(1e-3)
        host = m.sphere_sweep(kind, prims, rays)
        got = m.kat_sphere_sweep(kind, prims, rays)
        assert 0.2 < (host[0] != 0).mean() < 0.8 and not host[0][rows].any()
        for name, h, g in zip(("hit", "t", "centre", "point", "bary"), host, got):
            bad = (bits(h) != bits(g)).reshape(len(rays), -1).any(1) if h.dtype == f32 else h != g
            assert not bad.any(), "kind %d %s: %d of %d pairs differ, first %d: host %s device %s" % (
                kind, name, bad.sum(), len(rays), np.argmax(bad), h[np.argmax(bad)], g[np.argmax(bad)])


# ---- 2. a soup ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,size", [(0.0, 0.2), (1024.0, 0.01)])
def test_soup_under_both_accelerators(tmp_path, offset, size):
    import mobileraytracer_amd as m
    cfg = NB.obj_cfg(NB.soup(str(tmp_path), "soup", offset, size))
    geom = m.scene_triangles(cfg)[0]
    assert len(geom) == 300
    rays = C.scene_sweeps(geom, 600, 32, 1.0 + 2 * size)
    lists = C.Lists(cfg)
    times = lists.times(rays)
    bound = C.bounds_for(lists, rays, 33, times)
    want = lists.expected(rays, max_t=bound, times=times)
    free = lists.expected(rays, times=times)
    # (on the host) enough of each outcome, zero components of d, d = 0, r = 0, and bounds that cut contacts off
    moving, at0, missed = (want["hit"] == 1) & (want["t"] > 0), (want["hit"] == 1) & (want["t"] == 0), want["hit"] == 0
    print("soup at %g: %d hits with t > 0, %d at t = 0, %d misses; the bound cuts %d contacts off" % (
        offset, moving.sum(), at0.sum(), missed.sum(), (missed & (free["hit"] == 1)).sum()))
    assert moving.sum() >= 100 and at0.sum() >= 50 and missed.sum() >= 50
    assert (missed & (free["hit"] == 1)).sum() >= 20 and ((rays[:, 3:6] == 0).sum(1) == 2).sum() >= 100
    assert ((rays[:, 3:6] == 0).all(1)).sum() >= 100 and (rays[:, 6] == 0).sum() >= 20
    assert np.array_equal(bits(want["t"][missed]), bits(bound[missed])) and (want["index"][missed] == -1).all()
    both(cfg, rays, want, "soup at %g" % offset, max_t=bound)
    both(cfg, rays, free, "soup at %g, unbounded" % offset, accelerators=(BVH,))


# ---- 3. exact ties -----------------------------------------------------------------------------------
def test_exact_ties_go_to_the_kind_then_the_lowest_input_index(tmp_path):
    import mobileraytracer_amd as m
    cfg = NB.obj_cfg(NB.write_mesh(str(tmp_path), "sheets", quads=NB.sheet_quads(16, 0) + NB.sheet_quads(16, 2),
                                   light=NB.FAR_LIGHT))
    geom = m.scene_triangles(cfg)[0]
    assert len(geom) == 1024
    lo = NB.corners_of(geom).min(0)
    g = np.arange(33, dtype=f32) * f32(0.5)  # corners, edge midpoints and cell centres, midway between the sheets
    n = 33 * 33
    o = np.stack([lo[0] + np.repeat(g, 33), lo[1] + np.tile(g, 33), np.full(n, lo[2] + 1, f32)], 1).astype(f32)
    rng = np.random.default_rng(35)
    mode = np.arange(n) % 4  # 0, 1: starts touching both sheets; 2: moves up onto one; 3: down
    d = rng.normal(size=(n, 3)).astype(f32)
    d[mode == 2] = (0, 0, 2)
    d[mode == 3] = (0, 0, -4)
    rad = np.where(mode < 2, f32(1), f32(0.5)).astype(f32)
    rays = np.concatenate([o, d, rad[:, None]], 1).astype(f32)
    lists = C.Lists(cfg)
    t, hit = lists.times(rays)
    want = lists.expected(rays, times=(t, hit))
    assert (want["hit"] == 1).all() and (want["kind"] == C.TRIANGLE).all()
    assert (want["t"][mode < 2] == 0).all() and (want["t"][mode == 2] == 0.25).all() and (want["t"][mode == 3] == 0.125).all()
    tied = hit[:, :1024] & (t[:, :1024] == want["t"][:, None])
    ties = tied.sum(1)
    print("two sheets: %d of %d sweeps tie between two triangles or more, %d between four or more" % (
        (ties >= 2).sum(), n, (ties >= 4).sum()))
    assert (ties >= 1).all() and (ties >= 2).mean() > 0.9 and (ties >= 4).sum() >= 256  # (one triangle: at the rim)
    assert np.array_equal(want["index"], tied.argmax(1))  # (on the host) the lowest input index among them
    both(cfg, rays, want, "two sheets")


def test_a_plane_wins_a_tie_with_a_triangle():
    """A built-in scene with planes: a sphere that starts touching a plane and whatever else is at t = 0 is
    the plane's (kind 1 first), on the host and on the device."""
    import mobileraytracer_amd as m
    cfg = next(c for c in (m.Config(width=16, height=16, shader=1, sceneIndex=s) for s in (0, 1, 2, 3))
               if len(m.scene_planes(c)[0]) >= 1)
    lists = C.Lists(cfg)
    rng = np.random.default_rng(36)
    plane = lists.rec[C.PLANE][0]
    on = m.point_distance(C.PLANE, np.tile(plane, (128, 1)), rng.uniform(-2, 2, (128, 3)).astype(f32))[1]
    rays = np.concatenate([on, rng.normal(size=(128, 3)), np.full((128, 1), 64.0)], 1).astype(f32)  # touches everything near
    t, hit = lists.times(rays)
    want = lists.expected(rays, times=(t, hit))
    assert ((hit & (t == 0)).sum(1) >= 2).all() and (want["kind"] == C.PLANE).all() and (want["t"] == 0).all()
    both(cfg, rays, want, "a plane and more at t = 0")


# ---- 4. the cull -------------------------------------------------------------------------------------
def test_the_cull_skips_most_of_a_sheet(tmp_path):
    """The 46 x 46 sheet, short sweeps.  The bound on `tests` comes from the tree, not from the walk: a triangle
    can only be evaluated if, for some s in [0, bound], the centre is inside its leaf's box grown by the header's
    R - so the grown box overlaps the box of the centre's path (float64, a relative slack of 1e-4 on R)."""
    import mobileraytracer_amd as m
    cfg = NB.obj_cfg(NB.write_mesh(str(tmp_path), "sheet46", quads=NB.sheet_quads(46, 0), light=NB.FAR_LIGHT))
    geom = m.scene_triangles(cfg)[0]
    T = len(geom)
    assert T == 4232
    lo = NB.corners_of(geom).min(0)
    rng = np.random.default_rng(41)
    n = 512
    o = np.concatenate([lo[:2] + rng.integers(0, 46, (n, 2)) + rng.random((n, 2)), lo[2] + rng.uniform(0.3, 1.5, (n, 1))], 1)
    d = rng.normal(size=(n, 3))
    d *= rng.uniform(0.5, 2.0, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((n, 1), 0.25)], 1).astype(f32)
    bound = np.ones(n, f32)
    lists = C.Lists(cfg)
    F = lists.fixed
    assert F == 2
    want = lists.expected(rays, max_t=bound)
    assert 0.2 < want["hit"].mean() < 0.8
    boxes, _, cnt, _ = m.triangle_bvh(cfg)
    leaf = cnt > 0
    assert cnt[leaf].sum() == T
    b = boxes[leaf].astype(np.float64)
    p0, p1 = rays[:, :3].astype(np.float64), rays[:, :3].astype(np.float64) + rays[:, 3:6].astype(np.float64)
    mr = np.maximum(np.abs(p0).max(1), max(np.abs(boxes[0].astype(np.float64)).max(), 0.25))
    R = (C.cull_radius(0.25, mr) * (1 + 1e-4))[:, None, None]
    plo, phi = np.minimum(p0, p1)[:, None, :], np.maximum(p0, p1)[:, None, :]
    apart = ((b[None, :, :3] - R > phi) | (b[None, :, 3:] + R < plo)).any(2)
    reach = ((~apart) * cnt[leaf][None, :]).sum(1)
    got = both(cfg, rays, want, "sheet", max_t=bound)
    assert (got[NAIVE]["tests"] == T + F).all()  # Naive: every candidate
    tests, fast = got[BVH]["tests"], got[BVH, "hit"]["tests"]
    print("46 x 46 sheet, short sweeps: mean tests per sweep %.1f (hit only: %.1f), mean triangles in leaves within reach "
          "of the path %.1f (of %d)" % (tests.mean(), fast.mean(), reach.mean(), T))
    assert (tests >= F).all() and (tests - F <= reach).all()
    assert reach.mean() < T / 8  # (the bound says something)


# ---- 5. tree shapes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack%d" % S.STACK_DEEP, "degenerate", "inf_vertex", "outlier"])
def test_tree_shapes(tmp_path, name):
    import mobileraytracer_amd as m
    files = S.write_scene(str(tmp_path), name)
    cfg = NB.obj_cfg(files[:3])
    if name.startswith("stack"):
        assert m.walk_stack(cfg)["need"] == S.STACK_CASES[S.STACK_DEEP][1]  # far beyond the LDS stack
    rng = np.random.default_rng(51)
    geom = m.scene_triangles(cfg)[0]
    o = np.concatenate([rng.uniform((-9, -13, -11), (9, 10, 41), (128, 3)), NB.surface_points(geom, 64, rng, 0.5)])
    o = o[np.isfinite(o).all(1)]
    assert len(o) >= 160
    d = rng.normal(size=(len(o), 3)) * 10.0 ** rng.uniform(-1, 1.5, (len(o), 1))
    rad = 10.0 ** rng.uniform(-3, 0, (len(o), 1))
    rays = np.concatenate([o, d, rad], 1).astype(f32)
    want = C.Lists(cfg).expected(rays)
    assert not np.isnan(want["t"]).any() and 20 <= want["hit"].sum() <= len(o) - 5
    both(cfg, rays, want, name)


# ---- 6. the other kinds ------------------------------------------------------------------------------
def test_planes_spheres_triangles_and_lights():
    import mobileraytracer_amd as m
    seen, point_lights = set(), 0
    for scene in (0, 1, 2, 3):
        cfg = m.Config(width=16, height=16, shader=1, sceneIndex=scene)
        lists = C.Lists(cfg)
        nb = NB.Lists(cfg)
        rng = np.random.default_rng(60 + scene)
        o = NB.builtin_points(nb.cands, 256, 60 + scene)
        aim = NB.builtin_points(nb.cands, 256, 70 + scene)[rng.permutation(256)]
        rays = np.concatenate([o, (aim - o) * rng.uniform(0.5, 3.0, (256, 1)), 10.0 ** rng.uniform(-3, -0.5, (256, 1))], 1).astype(f32)
        want = lists.expected(rays)
        kinds = {k: int((want["kind"] == k).sum()) for k in (1, 2, 3, 4)}
        print("scene %d: candidates %s, answers per kind %s" % (scene, nb.cands.count, kinds))
        seen |= {k for k, c in kinds.items() if c >= 4}
        lkind = m.scene_lights(cfg)[0]
        point_lights += int((lkind == 0).sum())
        assert (lkind[want["index"][want["kind"] == C.LIGHT]] == 1).all()  # a point light never appears
        both(cfg, rays, want, "scene %d" % scene)
        # an accelerator id that builds nothing: the area lights only
        want0 = C.Lists(cfg, lights_only=True).expected(rays)
        assert set(np.unique(want0["kind"])) <= {0, C.LIGHT}
        both(cfg, rays, want0, "scene %d, no accelerator" % scene, accelerators=(0,))
    assert seen == {1, 2, 3, 4} and point_lights >= 1


# ---- 7. sources, batching and state ------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """shape_scenes' lit base (a frame of it is no single colour) and its candidates."""
    import mobileraytracer_amd as m
    cfg = NB.obj_cfg(S.write_base(str(tmp_path_factory.mktemp("sweep_base"))))
    return {"cfg": cfg, "geom": m.scene_triangles(cfg)[0], "lists": C.Lists(cfg)}


def test_a_sphere_resting_on_its_source_moves_freely_along_it(base):
    import mobileraytracer_amd as m
    geom, cfg, lists = base["geom"], base["cfg"], base["lists"]
    rng = np.random.default_rng(73)
    n = 256
    j = rng.integers(0, len(geom), n)
    w = np.array([(0.25, 0.25), (0.5, 0.25), (0.125, 0.5)], f32)[rng.integers(0, 3, n)]
    t = geom.reshape(-1, 9)[j]
    on = ((t[:, :3] + t[:, 3:6] * w[:, :1]) + t[:, 6:] * w[:, 1:]).astype(f32)  # exactly on triangle j (dyadic coordinates)
    nrm = np.cross(t[:, 3:6].astype(np.float64), t[:, 6:].astype(np.float64))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rad = np.full((n, 1), 0.0625)
    o = on + nrm * rad * (1 - 1e-3)  # resting on the triangle, pressed slightly into it
    d = t[:, 3:6] * rng.uniform(-0.2, 0.2, (n, 1)) + t[:, 6:] * rng.uniform(-0.2, 0.2, (n, 1))  # along the face
    rays = np.concatenate([o, d, rad], 1).astype(f32)
    times = lists.times(rays)
    free = lists.expected(rays, times=times)
    assert ((free["t"] == 0) & (free["hit"] == 1)).all()  # without a source the sphere is stuck where it starts
    src = np.stack([np.full(n, C.TRIANGLE), j], 1).astype(np.int32)
    want = lists.expected(rays, src=src, times=times)
    assert not ((want["kind"] == C.TRIANGLE) & (want["index"] == j)).any()
    assert ((want["hit"] == 0) | (want["t"] > 0)).mean() > 0.5  # ... with it, most move
    got = both(cfg, rays, want, "sources", src=src)
    assert not ((got[BVH]["kind"] == C.TRIANGLE) & (got[BVH]["index"] == j)).any()
    # a sphere or light source, a kind that is none, an index out of range: no source
    with m.Renderer(cfg) as r:
        for pair in ((C.SPHERE, 0), (C.LIGHT, 0), (C.LIGHT, 1), (C.TRIANGLE, 1 << 20), (C.TRIANGLE, -1), (C.PLANE, 0), (7, 0), (0, 0)):
            C.assert_same(sweep(r, rays, src=np.tile(np.array([pair], np.int32), (n, 1))), free, "src %s" % (pair,))


@pytest.fixture(scope="module")
def water():
    """tests/golden/CornellBox (Water) at 16 x 16: a small level-1 queue; n = 2 cap + 65 sweeps through a box
    about the scene, their bounds and the host's answers."""
    import mobileraytracer_amd as m
    cfg = water_cfg()
    with m.Renderer(cfg) as r:
        cap = r.queue_info()["rayCap"][0]
    assert cap >= 64
    boxes, _, _, _ = m.triangle_bvh(cfg)
    lo, hi = boxes[0, :3].astype(np.float64), boxes[0, 3:].astype(np.float64)
    n = 2 * cap + 65
    rng = np.random.default_rng(81)
    o = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (n, 3))
    d = rng.normal(size=(n, 3)) * (hi - lo).max() * 0.1
    rad = (hi - lo).max() * 10.0 ** rng.uniform(-3, -1.5, (n, 1))
    rays = np.concatenate([o, d, rad], 1).astype(f32)
    bound = np.where(rng.random(n) < 0.5, INF, rng.uniform(0.1, 4.0, n)).astype(f32)
    want = C.Lists(cfg).expected(rays, max_t=bound)
    assert 0.2 < want["hit"].mean() < 0.9 and len(np.unique(want["index"])) > 50
    rays.setflags(write=False)
    return {"cfg": cfg, "cap": cap, "rays": rays, "bound": bound, "want": want}


def test_chunks_a_stride_of_six_and_a_permuted_batch(water):
    import mobileraytracer_amd as m
    rays, bound, want = water["rays"], water["bound"], water["want"]
    perm = np.random.default_rng(82).permutation(len(rays))
    with m.Renderer(water["cfg"]) as r:
        got = sweep(r, rays, max_t=bound)
        strided = sweep(r, rays, max_t=bound, stride=6)
        permuted = sweep(r, rays[perm], max_t=bound[perm])
        assert r.queue_info()["rayCap"][0] == water["cap"]  # the chunking assumed
    C.assert_same(got, want, "2 cap + 65 sweeps")
    C.assert_same(strided, want, "stride 6")
    C.assert_same(permuted, C.rows_of(want, perm), "permuted")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches_and_single_fields_write_their_entries_and_nothing_else(water, n):
    import ctypes
    import torch
    import mobileraytracer_amd as m
    guard = 64
    want = {f: x[:n] for f, x in water["want"].items()}
    rays = water["rays"][:n]
    o, d, rad = dev(np.ascontiguousarray(rays[:, :3])), dev(np.ascontiguousarray(rays[:, 3:6])), dev(np.ascontiguousarray(rays[:, 6]))
    dist = dev(water["bound"][:n])

    def outputs():
        return {f: torch.full((guard + n * w + guard,), SENTINEL, dtype=torch.int32, device="cuda") for f, w in C.WIDTHS.items()}

    def check(out, wanted, what):
        for f, w in C.WIDTHS.items():
            x = out[f].cpu().numpy()
            assert (x[:guard] == SENTINEL).all() and (x[guard + n * w:] == SENTINEL).all(), (what, f)
            body = x[guard:guard + n * w]
            if f not in wanted:
                assert (body == SENTINEL).all(), (what, f)
            elif f != "tests":
                e = want[f] if want[f].dtype == np.int32 else bits(want[f])
                assert np.array_equal(body, e.reshape(-1)), (what, f)

    with m.Renderer(water["cfg"]) as r:
        for wanted in [ALL] + [(f,) for f in ALL]:
            out = outputs()
            torch.cuda.synchronize()
            r.sweep_spheres_device(o.data_ptr(), d.data_ptr(), rad.data_ptr(), n, d_dist=dist.data_ptr(),
                                   **{"d_" + f: out[f][guard:].data_ptr() for f in wanted})
            torch.cuda.synchronize()
            check(out, wanted, wanted)
        # a smaller outSize: the cut-off fields count as NULL
        out = outputs()
        torch.cuda.synchronize()
        r.sweep_spheres_device(o.data_ptr(), d.data_ptr(), rad.data_ptr(), n, d_dist=dist.data_ptr(),
                               out_size=3 * ctypes.sizeof(ctypes.c_void_p), **{"d_" + f: out[f][guard:].data_ptr() for f in ALL})
        torch.cuda.synchronize()
        check(out, ("hit", "kind", "index"), "outSize 24")


def test_a_query_leaves_frames_totals_and_ray_queries_alone(base):
    import mobileraytracer_amd as m
    cfg = dataclasses.replace(base["cfg"], width=32, height=32)
    rng = np.random.default_rng(91)
    o = np.stack([rng.uniform(-4, 4, 200), rng.uniform(-4, 4, 200), np.full(200, -9.0)], 1).astype(f32)
    d = np.stack([rng.uniform(-0.25, 0.25, 200), rng.uniform(-0.25, 0.25, 200), np.ones(200)], 1).astype(f32)
    rays = np.concatenate([o, d * 4, 10.0 ** rng.uniform(-2, 0, (200, 1))], 1).astype(f32)
    want = base["lists"].expected(rays)
    assert 0.2 < want["hit"].mean()

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
        got = sweep(r, rays)
        bytes1 = r.scene_info()["deviceBytes"]
        before = cast(r)
        again = sweep(r, rays, fields=("hit", "t"))
        after = cast(r)
        assert r.scene_info()["deviceBytes"] == bytes1  # no allocation after a renderer's first query
        assert r.get_total_casted_rays() == total
        now = r.frame_stats()
        assert all(now[k] == stats[k] for k in stats if not k.endswith("Ms"))
        b = frame(r)
        assert r.get_total_casted_rays() == ref_total
    C.assert_same(got, want, "between two frames")
    C.assert_same(again, want, "again", fields=("hit", "t"))
    for q in (before, after):
        assert np.array_equal(q[0], ref_cast[0]) and np.array_equal(q[1], ref_cast[1]) and np.array_equal(bits(q[2]), bits(ref_cast[2]))
    for x, y in ((a, ref[0]), (b, ref[1])):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2]
    assert a[1][0] > 0 and len(set(a[0].tolist())) > 1


def test_query_is_ordered_on_the_callers_stream(water):
    """On a stream of the caller's: a long run of kernels, then the kernel that fills the origins, then the
    query, then reductions of its outputs - and no synchronisation before the final copy."""
    import torch
    import mobileraytracer_amd as m
    rays = water["rays"]
    n = len(rays)
    src_o, dd, rad = dev(np.ascontiguousarray(rays[:, :3])), dev(np.ascontiguousarray(rays[:, 3:6])), dev(np.ascontiguousarray(rays[:, 6]))
    dist = dev(water["bound"])
    want = [dev(x) for x in (water["want"]["hit"], water["want"]["index"], bits(water["want"]["t"]))]
    busy = torch.ones(1 << 24, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with m.Renderer(water["cfg"]) as r:
        with torch.cuda.stream(stream):
            o = torch.zeros(n, 3, device="cuda")
            h = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
            i = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
            t = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
            for _ in range(200):
                busy.mul_(1.0001)
            o.add_(src_o)
            r.sweep_spheres_device(o.data_ptr(), dd.data_ptr(), rad.data_ptr(), n, d_dist=dist.data_ptr(), d_hit=h.data_ptr(),
                                   d_index=i.data_ptr(), d_t=t.data_ptr(), stream=stream.cuda_stream)
            wrong = (h != want[0]).sum() + (i != want[1]).sum() + (t != want[2]).sum()
            wrong = int(wrong.cpu())  # (the first wait for the device)
    assert wrong == 0


def test_regular_grid_and_device_groups_are_refused(base):
    import torch
    import mobileraytracer_amd as m
    o = dev(np.zeros((70, 3), f32))
    d = dev(np.ones((70, 3), f32))
    rad = dev(np.full(70, 0.25, f32))
    hit = torch.full((70,), SENTINEL, dtype=torch.int32, device="cuda")
    for cfg, message in ((dataclasses.replace(base["cfg"], accelerator=GRID), "RegularGrid"),
                         (m.Config(width=16, height=16, shader=1, sceneIndex=0, devices=[0, 0]), "device groups are not supported")):
        with m.Renderer(cfg) as r:
            total = r.get_total_casted_rays()
            with pytest.raises(RuntimeError, match=message):
                r.sweep_spheres_device(o.data_ptr(), d.data_ptr(), rad.data_ptr(), 70, d_hit=hit.data_ptr())
            with pytest.raises(RuntimeError, match=message):
                r.sweep_spheres(o, d, rad)
            torch.cuda.synchronize()
            assert (hit.cpu().numpy() == SENTINEL).all() and r.get_total_casted_rays() == total


# ---- the wrapper -------------------------------------------------------------------------------------
def test_wrapper_handles_tensors_empty_batches_and_bad_fields(water):
    import torch
    import mobileraytracer_amd as m
    rays, want = water["rays"][:70], {f: x[:70] for f, x in water["want"].items()}
    rows = dev(np.ascontiguousarray(rays[:, :6]))
    rad, dist = dev(np.ascontiguousarray(rays[:, 6])), dev(water["bound"][:70])
    with m.Renderer(water["cfg"]) as r:
        assert r.SWEEP_FIELDS == ALL
        got = r.sweep_spheres(rows[:, :3], rows[:, 3:], rad, max_t=dist)  # two column slices of one (n, 6) tensor
        assert set(got) == set(ALL) and got["centre"].shape == (70, 3) and got["t"].dtype == torch.float32
        C.assert_same({f: x.cpu().numpy() for f, x in got.items()}, want, "the wrapper")
        empty = r.sweep_spheres(rows[:0, :3], rows[:0, 3:], rad[:0])
        assert set(empty) == set(ALL) and empty["hit"].shape == (0,) and empty["point"].shape == (0, 3)
        only = r.sweep_spheres(rows[:, :3], rows[:, 3:], rad, max_t=dist, fields=("hit",))
        assert set(only) == {"hit"} and np.array_equal(only["hit"].cpu().numpy(), want["hit"])
        for bad in (("depth",), ()):
            with pytest.raises(ValueError):
                r.sweep_spheres(rows[:, :3], rows[:, 3:], rad, fields=bad)
        with pytest.raises(ValueError):
            r.sweep_spheres(rows[:, :3], rows[:, 3:], rad[:5])
        with pytest.raises(TypeError):
            r.sweep_spheres_device(rows.data_ptr(), rows.data_ptr(), rad.data_ptr(), 70, d_normal=rows.data_ptr())
