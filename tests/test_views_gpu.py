"""Batches of views (mrt_render_views): K cameras of one scene rendered as one wavefront over
K x pixelSlots virtual slots.  The contract is bit-equality with set_camera + render_frame per view,
so every check here is exact: bitmaps, ray counts, per-level counts.

Every bitmap starts filled with a sentinel, so a pixel written into the wrong view's image, or not
written at all, shows up.
"""
import ctypes
import dataclasses
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = np.int32(0x12345678)  # alpha 0x12: never produced by incrementalAvg (alpha 0xFF)
WHITTED, PATH_TRACER = 1, 2
W, H = 64, 48
N = W * H
UP = (0.0, 1.0, 0.0)
# built-in scene 0 (the Cornell box, [-1, 1]^3 seen from z < 0): two perspective cameras and an
# orthographic one between them, all distinct, so a batch mixes camera kinds
CAMS = [
    (0, (0.4, 0.2, -3.0), (0.0, 0.0, 1.0), UP, 50.0, 40.0),
    (1, (0.1, -0.1, -2.0), (0.0, 0.0, 1.0), UP, 2.2, 1.8),
    (0, (-0.6, 0.3, -2.6), (0.1, -0.1, 1.0), UP, 60.0, 45.0),
]
K = len(CAMS)


def cornell_cfg(shader, spp=1, progressive=0, **kw):
    import mobileraytracer_amd as m
    return m.Config(width=W, height=H, shader=shader, sceneIndex=0, samplesPixel=spp, progressive=progressive, **kw)


def sentinel(*shape):
    return np.full(shape, SENTINEL, np.int32)


@functools.lru_cache(maxsize=None)
def singles(shader, spp, progressive):
    """Per view of CAMS: set_camera + render_frame on one renderer (the whole frame, one rank).
    Returns (bitmaps (K, N), rays per view, counts() per view), computed once and shared."""
    import mobileraytracer_amd as m
    bms, rays, levels = sentinel(K, N), [], []
    with m.Renderer(cornell_cfg(shader, spp, progressive)) as r:
        for v, cam in enumerate(CAMS):
            before = r.get_total_casted_rays()
            r.set_camera(*cam)
            r.render_frame(bms[v])
            rays.append(r.get_total_casted_rays() - before)
            levels.append(counts(r))
    assert not (bms == SENTINEL).any()
    assert len({bms[v].tobytes() for v in range(K)}) == K  # three different images
    bms.setflags(write=False)
    return bms, tuple(rays), tuple(levels)


def counts(r):
    """The last frame's (or batch's) ray counts: per level, per level's shadow rays, primary."""
    st = r.frame_stats()
    return tuple(st["levelRays"]) + tuple(st["levelShadowRays"]) + (st["primaryRays"], st["rays"], st["shadowRays"])


def level_sum(levels):
    return tuple(sum(x) for x in zip(*levels))


# ---- 1. a batch equals its single frames ------------------------------------------------------------
@pytest.mark.parametrize("progressive", [0, 1])
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
def test_batch_equals_single_frames(shader, spp, progressive):
    import mobileraytracer_amd as m
    ref, ref_rays, ref_levels = singles(shader, spp, progressive)
    with m.Renderer(cornell_cfg(shader, spp, progressive)) as r:
        own = sentinel(N)
        r.render_frame(own)  # the renderer's own camera, before the batch
        own_rays = r.get_total_casted_rays()
        bms = sentinel(K, N)
        r.render_views(CAMS, bms)
        for v in range(K):
            assert np.array_equal(bms[v], ref[v]), "view %d differs from its single frame" % v
        assert r.get_total_casted_rays() == own_rays + sum(ref_rays)
        st = r.frame_stats()
        assert counts(r) == level_sum(ref_levels)
        assert st["rays"] + st["shadowRays"] == sum(ref_rays) and st["levelRays"][0] == K * N * spp
        assert r.get_sample() == spp
        # the renderer's own camera is unchanged
        again = sentinel(N)
        r.render_frame(again)
        assert np.array_equal(again, own)
        assert r.get_total_casted_rays() == 2 * own_rays + sum(ref_rays)


def test_batch_of_one_view_is_that_frame():
    import mobileraytracer_amd as m
    ref, ref_rays, _ = singles(PATH_TRACER, 3, 0)
    with m.Renderer(cornell_cfg(PATH_TRACER, 3)) as r:
        bm = sentinel(1, N)
        r.render_views(CAMS[1:2], bm)
        assert np.array_equal(bm[0], ref[1]) and r.get_total_casted_rays() == ref_rays[1]


# ---- 2. parity with the CPU oracle ------------------------------------------------------------------
# glassboxes, the camera inside the innermost cube; values exact in float32, so the .cam text and the
# views hold the same numbers
GLASS = 64
GLASS_CAMS = [  # position, lookAt, (f.u, f.v) of the .cam file
    ((0.25, 0.125, 0.5), (0.0, 0.0, -1.0), (60.0, 60.0)),
    ((-0.375, -0.25, 0.25), (0.5, 0.25, -1.0), (50.0, 45.0)),
    ((0.125, 0.375, -0.25), (-1.0, 0.0, 0.25), (70.0, 55.0)),
]


def glass_views():
    """The views that loadCameraStream makes of GLASS_CAMS: position X negated, hFov = f.u * ratio in
    float32 (ratio 1 at 64 x 64)."""
    ratio = np.float32(GLASS) / np.float32(GLASS)
    return [(0, (-p[0], p[1], p[2]), l, UP, float(np.float32(f[0]) * ratio), f[1]) for p, l, f in GLASS_CAMS]


def glass_cfg(shader, spp=1, progressive=0):
    import mobileraytracer_amd as m
    from mobileraytracer_amd import scenes
    obj, mtl, cam = scenes.glass_boxes()
    return m.Config(width=GLASS, height=GLASS, shader=shader, samplesPixel=spp, samplesLight=1, maxDepth=4,
                    sceneIndex=-1, objFilePath=obj, mtlFilePath=mtl, camFilePath=cam, progressive=progressive)


@pytest.fixture(scope="module")
def glass_oracle(oracle_mod, tmp_path_factory):
    """(shader, spp) -> (bitmaps (K, n), rays per view) of the CPU oracle, one .cam file per view;
    rendered once per configuration and shared."""
    from mobileraytracer_amd import scenes
    obj, mtl, _ = scenes.glass_boxes()
    d = tmp_path_factory.mktemp("views_cams")
    paths = []
    for v, (p, l, f) in enumerate(GLASS_CAMS):
        path = d / ("view%d.cam" % v)
        path.write_text("t perspective\np %r %r %r\nl %r %r %r\nu 0 1 0\nf %r %r\n" % (*p, *l, *f))
        paths.append(str(path))
    cache = {}

    def get(shader, spp):
        if (shader, spp) not in cache:
            bms, rays = sentinel(K, GLASS * GLASS), []
            for v, path in enumerate(paths):
                o = oracle_mod.Oracle(GLASS, GLASS, shader, -1, spp, 1, 4, obj=obj, mtl=mtl, cam=path)
                rays.append(o.render(bms[v], threads=min(16, os.cpu_count() or 1))[1])
                o.close()
            assert len({bms[v].tobytes() for v in range(K)}) == K
            bms.setflags(write=False)
            cache[(shader, spp)] = (bms, tuple(rays))
        return cache[(shader, spp)]
    return get


@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
def test_batch_is_bit_equal_to_the_oracle(glass_oracle, shader):
    import mobileraytracer_amd as m
    ref, ref_rays = glass_oracle(shader, 1)
    with m.Renderer(glass_cfg(shader)) as r:
        bms = sentinel(K, GLASS * GLASS)
        r.render_views(glass_views(), bms)
        for v in range(K):
            assert np.array_equal(bms[v], ref[v]), "view %d differs from the oracle" % v
        assert r.get_total_casted_rays() == sum(ref_rays)


# ---- 3. waves that straddle views -------------------------------------------------------------------
def render_rank_batches(shader, spp, tuning=(), progressive=0):
    """The batch on each of 3 rank shards (86 / 85 / 85 units of 4 x 3 pixels: 1032 / 1020 / 1020
    slots, no multiple of 64, so every view boundary lies inside a wave), merged on the host.
    Returns (merged bitmaps, rays summed over the ranks, levelRays summed)."""
    import mobileraytracer_amd as m
    merged, rays, levels = sentinel(K, N), 0, []
    for k in range(3):
        with m.Renderer(cornell_cfg(shader, spp, progressive, rankIndex=k, rankCount=3)) as r:
            slots = r.scene_info()["pixelSlots"]
            assert slots % 64 != 0 and (slots * spp) % 64 != 0, slots  # the precondition: straddling waves
            for key, value in tuning:
                r.set_tuning(key, value)
            bms = sentinel(K, N)
            r.render_views(CAMS, bms)
            mine = bms != SENTINEL
            assert (mine.sum(axis=1) == slots).all()  # its own pixels of every view, nothing else
            assert not (mine & (merged != SENTINEL)).any()
            merged[mine] = bms[mine]
            rays += r.get_total_casted_rays()
            levels.append(counts(r))
    return merged, rays, level_sum(levels)


# key 17: level 1 fused (1) or in separate launches (0); key 33 (unfused): camera rays from k_raygen
# (0), generated and stored by the packet walk (1), regenerated in k_shade (2); key 34: level 1's
# resolve folded into the accumulation (1) or k_accumulate (0)
@pytest.mark.parametrize("shader,spp,fuse,gen,resolve_acc", [
    (PATH_TRACER, 1, 0, 0, 1), (PATH_TRACER, 1, 0, 1, 1), (PATH_TRACER, 1, 0, 2, 1), (PATH_TRACER, 1, 1, 2, 1),
    (PATH_TRACER, 1, 0, 2, 0), (PATH_TRACER, 1, 1, 2, 0),
    (WHITTED, 3, 0, 2, 1), (WHITTED, 3, 1, 1, 1),
])
def test_rank_shards_put_two_views_in_one_wave(shader, spp, fuse, gen, resolve_acc):
    ref, ref_rays, ref_levels = singles(shader, spp, 0)
    merged, rays, levels = render_rank_batches(shader, spp, ((17, fuse), (33, gen), (34, resolve_acc)))
    for v in range(K):
        assert np.array_equal(merged[v], ref[v]), "view %d differs from its single frame" % v
    assert rays == sum(ref_rays) and levels == level_sum(ref_levels)


def test_rank_shards_progressive():
    ref, ref_rays, _ = singles(PATH_TRACER, 3, 1)
    merged, rays, _ = render_rank_batches(PATH_TRACER, 3, progressive=1)
    assert np.array_equal(merged, ref) and rays == sum(ref_rays)


@pytest.mark.parametrize("shader,spp,budget,fuse", [(PATH_TRACER, 3, 12000, 1), (WHITTED, 1, 4000, 0),
                                                     (PATH_TRACER, 1, 1000, 1)])
def test_chunks_that_cut_views(shader, spp, budget, fuse):
    """maxPathsPerPass below the batch's paths: several chunks, whose ends lie inside views (and, the
    chunk being no multiple of 64 paths or the view no multiple of the chunk, inside waves)."""
    import mobileraytracer_amd as m
    ref, ref_rays, ref_levels = singles(shader, spp, 0)
    with m.Renderer(cornell_cfg(shader, spp, maxPathsPerPass=budget)) as r:
        r.set_tuning(17, fuse)
        slots = r.scene_info()["pixelSlots"]
        bms = sentinel(K, N)
        r.render_views(CAMS, bms)
        q = r.queue_info()
        print("queue info of the batch", {k: q[k] for k in ("chunkSlots", "passes")}, "pixelSlots", slots)
        assert q["passes"] > 1 and q["chunkSlots"] % slots != 0 and slots % q["chunkSlots"] != 0
        assert q["chunkSlots"] * q["passes"] >= K * slots > q["chunkSlots"] * (q["passes"] - 1)
        for v in range(K):
            assert np.array_equal(bms[v], ref[v]), "view %d differs from its single frame" % v
        assert r.get_total_casted_rays() == sum(ref_rays)
        assert counts(r) == level_sum(ref_levels)


# ---- 4. packed output -------------------------------------------------------------------------------
def test_packed_output_is_view_major():
    import torch
    import mobileraytracer_amd as m
    ref, _, _ = singles(PATH_TRACER, 1, 0)
    stream = torch.cuda.current_stream().cuda_stream
    merged = sentinel(K, N)
    for k in range(3):
        with m.Renderer(cornell_cfg(PATH_TRACER, 1, rankIndex=k, rankCount=3)) as r:
            slots = r.scene_info()["pixelSlots"]
            want = torch.full((K, slots), int(SENTINEL), dtype=torch.int32, device="cuda")
            for v, cam in enumerate(CAMS):
                r.set_camera(*cam)
                r.render_frame_device(0, want[v].data_ptr(), stream)
            packed = torch.full((K * slots + 64,), int(SENTINEL), dtype=torch.int32, device="cuda")
            d_bms = torch.full((K, N), int(SENTINEL), dtype=torch.int32, device="cuda")
            r.render_views_device(CAMS, d_bms.data_ptr(), packed.data_ptr(), stream)
            torch.cuda.synchronize()
            got = packed.cpu().numpy()
            assert (got[K * slots:] == SENTINEL).all()  # nothing past views x pixelSlots
            assert np.array_equal(got[:K * slots].reshape(K, slots), want.cpu().numpy())
            assert not (got[:K * slots] == SENTINEL).any()
            bms = d_bms.cpu().numpy()
            mine = bms != SENTINEL
            assert (mine.sum(axis=1) == slots).all()
            merged[mine] = bms[mine]
            # the packed buffer alone
            packed2 = torch.full((K * slots,), int(SENTINEL), dtype=torch.int32, device="cuda")
            r.render_views_device(CAMS, 0, packed2.data_ptr(), stream)
            torch.cuda.synchronize()
            assert torch.equal(packed2, packed[:K * slots])
    assert np.array_equal(merged, ref)


# ---- 5. replanning inside a batch -------------------------------------------------------------------
@pytest.mark.parametrize("shader,spp,progressive", [(WHITTED, 1, 0), (PATH_TRACER, 1, 0), (PATH_TRACER, 2, 1)])
def test_batch_overflows_replans_and_still_matches_the_oracle(glass_oracle, shader, spp, progressive):
    """The first allocation cut to a quarter of level 1 with no slack (tuning keys 38, 39): the batch's
    pass overflows, is replanned from what it asked for and redone; in progressive mode the running
    average of all the views is restored before the redo."""
    import mobileraytracer_amd as m
    ref, ref_rays = glass_oracle(shader, spp)
    with m.Renderer(glass_cfg(shader, spp, progressive)) as r:
        r.set_tuning(38, 25)
        r.set_tuning(39, 0)
        bms = sentinel(K, GLASS * GLASS)
        r.render_views(glass_views(), bms)
        q = r.queue_info()
        print("replanned batch", {k: q[k] for k in ("chunkSlots", "passes", "replansLastFrame", "worstCase")})
        assert q["replansLastFrame"] >= 1
        for v in range(K):
            assert np.array_equal(bms[v], ref[v]), "view %d differs from the oracle" % v
        assert r.get_total_casted_rays() == sum(ref_rays)
        assert r.get_sample() == spp


# ---- 6. device groups are refused -------------------------------------------------------------------
def test_device_group_refuses_a_batch():
    import mobileraytracer_amd as m
    cfg = cornell_cfg(WHITTED)
    with m.Renderer(cfg) as r:
        want = sentinel(N)
        r.render_frame(want)
        rays = r.get_total_casted_rays()
    with m.Renderer(dataclasses.replace(cfg, devices=[0, 0])) as g:
        bms = sentinel(K, N)
        with pytest.raises(RuntimeError, match="device groups are not supported"):
            g.render_views(CAMS, bms)
        assert (bms == SENTINEL).all() and g.get_total_casted_rays() == 0
        with pytest.raises(RuntimeError, match="device groups are not supported"):
            g.render_views_device(CAMS, 1, 0)  # (refused before the pointer is looked at)
        bm = sentinel(N)
        g.render_frame(bm)
        assert np.array_equal(bm, want) and g.get_total_casted_rays() == rays


# ---- 7. a batch beyond the int range ----------------------------------------------------------------
def test_batch_beyond_the_slot_range_is_refused():
    import mobileraytracer_amd as m
    from mobileraytracer_amd import _native
    with m.Renderer(cornell_cfg(WHITTED)) as r:
        slots = r.scene_info()["pixelSlots"]
        n = (1 << 31) // slots + 1  # n x pixelSlots >= 2^31
        views = (_native.MrtView * n).from_buffer_copy(bytes(r._views(CAMS[:1])[0]) * n)
        out = sentinel(N)
        assert _native.lib().mrt_render_views(r._h, views, n, out.ctypes.data_as(ctypes.c_void_p)) == -1
        assert b"beyond" in _native.lib().mrt_last_error()
        assert (out == SENTINEL).all() and r.get_total_casted_rays() == 0
