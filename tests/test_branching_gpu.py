"""Ray trees of any branching: the wavefront queues are planned from what an overflowed pass asked
for (mrt_queue_plan.hpp), so a scene whose levels outgrow twice the camera rays renders, bit-equal to
the oracle, instead of failing with "wavefront queue overflow persists".

The scene: tests/golden/glassboxes (scenes.glass_boxes()) - three nested glass cubes whose every hit
spawns a diffuse, a specular and a transmitted ray.  CPU oracle, depth 6, 1 spp: 136 casts per pixel
under Whitted, 559 under PathTracer; the deepest level holds more than 16 x (Whitted) and 80 x
(PathTracer) the camera rays, where the fixed allocation held 2 x plus 3072 slots per segment.
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


def glass_cfg(width, height, shader, spp=1, **kw):
    import mobileraytracer_amd as m
    from mobileraytracer_amd import scenes
    obj, mtl, cam = scenes.glass_boxes()
    return m.Config(width=width, height=height, shader=shader, samplesPixel=spp, samplesLight=1, maxDepth=6,
                    sceneIndex=-1, objFilePath=obj, mtlFilePath=mtl, camFilePath=cam, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_frame(width, height, shader, spp, scene_index):
    """(bitmap, casted rays) of the CPU oracle, rendered once per configuration and shared."""
    from oracle import oracle as O
    from mobileraytracer_amd import scenes
    obj, mtl, cam = scenes.glass_boxes() if scene_index < 0 else ("", "", "")
    o = O.Oracle(width, height, shader, scene_index, spp, 1, 6, obj=obj, mtl=mtl, cam=cam)
    bm = np.full(width * height, SENTINEL, np.int32)
    _, rays = o.render(bm, threads=min(16, os.cpu_count() or 1))
    o.close()
    bm.setflags(write=False)
    return bm, rays


def oracle_frame(cfg):
    return _oracle_frame(cfg.width, cfg.height, cfg.shader, cfg.samplesPixel, cfg.sceneIndex)


def render(r, cfg):
    bm = np.full(cfg.width * cfg.height, SENTINEL, np.int32)
    r.render_frame(bm)
    return bm


@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
def test_glassboxes_renders_bit_equal_to_the_oracle(oracle_mod, shader):
    import mobileraytracer_amd as m
    cfg = glass_cfg(128, 128, shader)
    ref, ref_rays = oracle_frame(cfg)
    with m.Renderer(cfg) as r:
        first_alloc = r.queue_info()
        bm = render(r, cfg)
        assert np.array_equal(bm, ref)
        assert r.get_total_casted_rays() == ref_rays
        level = r.frame_stats()["levelRays"]
        print("levelRays", level[:7], "per camera ray", [round(x / level[0], 2) for x in level[:7]])
        assert level[0] == 128 * 128 and max(level[1:7]) > 2 * level[0]
        q = r.queue_info()
        print("queue info after frame 1", q)
        assert q["replansLastFrame"] >= 1 and q["replans"] == q["replansLastFrame"]
        # the plan holds what the pass asked for, level by level, where the first allocation did not
        assert max(q["requestedRays"][:7]) > max(first_alloc["rayCap"][:7])
        # (levels 1-6; the depth-capped level 7's rays are counted, never written: no capacity needed)
        for lv in range(6):
            assert q["rayCap"][lv] >= q["requestedRays"][lv] > 0
            assert q["shadowCap"][lv] >= q["requestedShadows"][lv]
        assert q["requestedRays"][:7] == level[:7]  # one chunk: the pass's totals are the frame's
        assert q["queueBytes"] <= q["budgetBytes"]
        # the learned plan stays with the renderer: the next frame does not retry
        bm2 = render(r, cfg)
        assert np.array_equal(bm2, ref)
        q2 = r.queue_info()
        assert q2["replansLastFrame"] == 0 and q2["replans"] == q["replans"]
        assert q2["rayCap"] == q["rayCap"] and q2["chunkSlots"] == q["chunkSlots"]
        assert r.get_total_casted_rays() == 2 * ref_rays


def test_progressive_frame_keeps_its_average_across_a_replanned_sample(oracle_mod):
    """One pass per sample; the running average is backed up before a sample and restored when the
    sample's pass overflowed and is redone."""
    import mobileraytracer_amd as m
    cfg = glass_cfg(64, 64, PATH_TRACER, spp=3, progressive=1)
    ref, ref_rays = oracle_frame(cfg)
    with m.Renderer(cfg) as r:
        bm = render(r, cfg)
        q = r.queue_info()
        assert q["replansLastFrame"] >= 1
        assert np.array_equal(bm, ref) and r.get_total_casted_rays() == ref_rays
        assert r.get_sample() == 3
    # the bitmap after sample 1: a progressive frame that ends there is the 1-spp frame (a 3-spp
    # frame's first sample is jittered by the Halton pixel sampler, a 1-spp frame's by the constant
    # one, C_wrapper.cpp:144-148, so the two are compared at 1 spp)
    cfg1 = glass_cfg(64, 64, PATH_TRACER, spp=1, progressive=1)
    ref1, ref1_rays = oracle_frame(cfg1)
    with m.Renderer(cfg1) as r:
        bm = render(r, cfg1)
        assert r.queue_info()["replansLastFrame"] >= 1 and r.get_sample() == 1
        assert np.array_equal(bm, ref1) and r.get_total_casted_rays() == ref1_rays


def test_two_shards_replan_each_for_itself(oracle_mod):
    import torch
    import mobileraytracer_amd as m
    cfg = glass_cfg(128, 128, WHITTED)
    with m.Renderer(cfg) as r:
        single = render(r, cfg)
        rays = r.get_total_casted_rays()
    assert np.array_equal(single, oracle_frame(cfg)[0])
    # two ranks, each its packed half, assembled by rank 0
    rs = [m.Renderer(dataclasses.replace(cfg, rankIndex=k, rankCount=2)) for k in range(2)]
    try:
        slots_max = rs[0].scene_info()["pixelSlotsMax"]
        gathered = torch.zeros((2, slots_max), dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for k, r in enumerate(rs):
            r.render_frame_device(0, gathered[k].data_ptr(), stream)
        torch.cuda.synchronize()
        out = torch.full((128 * 128,), int(SENTINEL), dtype=torch.int32, device="cuda")
        rs[0].unpack_gathered(gathered.data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), single)
        assert sum(r.get_total_casted_rays() for r in rs) == rays
        assert all(r.queue_info()["replansLastFrame"] >= 1 for r in rs)
    finally:
        for r in rs:
            r.close()
    # a device group of two shards on one GPU
    with m.Renderer(dataclasses.replace(cfg, devices=[0, 0])) as g:
        bm = render(g, cfg)
        assert np.array_equal(bm, single) and g.get_total_casted_rays() == rays
        q = g.queue_info()
        assert q["replansLastFrame"] >= 2  # summed over the shards: each planned for itself
        bm = render(g, cfg)
        assert np.array_equal(bm, single) and g.queue_info()["replansLastFrame"] == 0


def test_forced_replan_on_an_ordinary_scene():
    """The retry path on a scene the first allocation holds: the built-in Cornell box with the first
    allocation cut to a quarter of level 1 and no slack (tuning keys 38, 39)."""
    import mobileraytracer_amd as m
    cfg = m.Config(width=64, height=64, shader=PATH_TRACER, sceneIndex=0, samplesPixel=2)
    with m.Renderer(cfg) as r:
        want = render(r, cfg)
        st = r.frame_stats()
        q0 = r.queue_info()
        assert q0["replans"] == 0 and r.get_tuning(38) == 200 and r.get_tuning(39) == 3072 and r.get_tuning(37) == 0
    with m.Renderer(cfg) as r:
        r.set_tuning(38, 25)
        r.set_tuning(39, 0)
        bm = render(r, cfg)
        st2 = r.frame_stats()
        q = r.queue_info()
        print("forced replan", q)
        assert np.array_equal(bm, want)
        assert st2["rays"] == st["rays"] and st2["shadowRays"] == st["shadowRays"]
        assert st2["levelRays"] == st["levelRays"] and st2["levelShadowRays"] == st["levelShadowRays"]
        assert q["replansLastFrame"] >= 1 and not q["worstCase"]
        bm = render(r, cfg)
        assert np.array_equal(bm, want) and r.queue_info()["replansLastFrame"] == 0


def test_forced_small_budget_renders_in_chunks(oracle_mod):
    """A 64 MiB queue budget (tuning key 37): the first allocation fits it, the plan for what
    glassboxes asks for under PathTracer does not, so the frame renders in several chunks (or under
    the worst-case plan's chunk)."""
    import mobileraytracer_amd as m
    cfg = glass_cfg(32, 32, PATH_TRACER)
    ref, ref_rays = oracle_frame(cfg)
    with m.Renderer(cfg) as r:
        r.set_tuning(37, 64)
        bm = render(r, cfg)
        q = r.queue_info()
        print("small budget", q)
        assert np.array_equal(bm, ref) and r.get_total_casted_rays() == ref_rays
        assert q["budgetBytes"] == 64 << 20 and q["queueBytes"] <= q["budgetBytes"]
        assert q["passes"] > 1
        assert q["worstCase"] or q["chunkSlots"] < 32 * 32
        assert q["replansLastFrame"] >= 1


def test_queue_info_copies_at_most_size_bytes():
    import mobileraytracer_amd as m
    from mobileraytracer_amd import _native
    full = ctypes.sizeof(_native.MrtQueueInfo)
    cfg = m.Config(width=32, height=32, shader=WHITTED, sceneIndex=0)
    with m.Renderer(cfg) as r:
        want = r.queue_info()
        for size in (0, 8, 24, full, full + 64):
            buf = (ctypes.c_uint8 * (full + 64))(*([0x5A] * (full + 64)))
            assert _native.lib().mrt_get_queue_info(r._h, ctypes.cast(buf, ctypes.c_void_p), size) == 0
            raw = bytes(buf)
            n = min(size, full)
            assert raw[n:] == b"\x5a" * (full + 64 - n), size  # nothing past `size`, nor past the struct
            got = _native.MrtQueueInfo.from_buffer_copy(raw[:full])
            if size >= 24:
                assert (got.chunkSlots, got.passes, got.queueBytes) == (want["chunkSlots"], want["passes"],
                                                                       want["queueBytes"])
            if size == 8:
                assert got.chunkSlots == want["chunkSlots"] == 32 * 32
                assert got.passes == 0x5A5A5A5A5A5A5A5A  # the guard pattern, untouched
