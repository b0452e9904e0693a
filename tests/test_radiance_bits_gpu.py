"""Shaded radiance as float bits, and ray trees to the depth limit.

shade_rays promises linear float RGB per ray, bit-equal to what Shader::rayTrace hands to the pixel
average.  The frame tests cannot see that: a pixel is the radiance clamped to [0, 1] and truncated to
0..255, so an error below 1/255, an error in a channel above 1 and nearly everything a deep level
contributes are invisible in it (glassboxes, Whitted, depth 12 -> 13: no pixel of the 8-bit frame
changes, the float radiance of every camera ray does).  Here the int32 view of Renderer.shade_rays is
compared with the int32 view of Oracle.shade_rays (tests/test_oracle_radiance_cpu.py pins that one to
the oracle's frame), every ray and every channel, and the frames run at maxDepth 7 .. 13, the limit.

Before any GPU comparison each case checks on the oracle's output alone that it is not vacuous: at
least half of the rays carry radiance, and all of it is finite.
"""
import dataclasses
import functools
import time

import numpy as np
import pytest

import texture_scenes as T
from test_cast_rays_gpu import mixed_rays
from test_oracle_radiance_cpu import THREADS, bits, teapot_from_above

pytestmark = pytest.mark.gpu

SENTINEL = 0x12345678  # as int32: alpha 0x12, never produced by incrementalAvg; as float32 bits: 5.69e-28
WHITTED, PATH_TRACER, DEPTH_MAP, DIFFUSE, NO_SHADOWS = 1, 2, 3, 4, 5
SIZE = 16


def config(scene, shader=WHITTED, spp=1, spl=1, depth=6, size=SIZE, **kw):
    """scene: a built-in scene's index, "water" / "glassboxes", or an (obj, mtl, cam) triple."""
    import mobileraytracer_amd as m
    from mobileraytracer_amd import scenes
    common = dict(width=size, height=size, shader=shader, samplesPixel=spp, samplesLight=spl, maxDepth=depth, **kw)
    if isinstance(scene, int):
        return m.Config(sceneIndex=scene, **common)
    obj, mtl, cam = {"water": scenes.cornell_water, "glassboxes": scenes.glass_boxes}[scene]() if isinstance(scene, str) else scene
    return m.Config(sceneIndex=-1, objFilePath=obj, mtlFilePath=mtl, camFilePath=cam, **common)


def oracle_of(oracle_mod, cfg):
    return oracle_mod.Oracle(cfg.width, cfg.height, cfg.shader, cfg.sceneIndex, cfg.samplesPixel, cfg.samplesLight,
                             cfg.maxDepth, obj=cfg.objFilePath, mtl=cfg.mtlFilePath, cam=cfg.camFilePath,
                             accelerator=cfg.accelerator)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int32) if a.dtype == np.uint32 else a).copy()).cuda()  # (a copy: shared batches are read-only)


def host(t):
    """A float32 / int32 / uint32 tensor's bits on the host as int32."""
    import torch
    return t.contiguous().view(torch.int32).cpu().numpy()


def oracle_radiance(oracle_mod, cfg, rays=None, src=None, min_bright=0):
    """The reference side of one case: (orig, dirs, keys, radiance, casts, seconds) of ``rays`` (None: the
    configuration's camera rays), refused where the case would be vacuous."""
    ob = oracle_of(oracle_mod, cfg)
    orig, dirs, keys = ob.camera_rays()[:3] if rays is None else rays
    t0 = time.perf_counter()
    want, casts = ob.shade_rays(orig, dirs, keys, src, threads=THREADS)
    seconds = time.perf_counter() - t0
    ob.close()
    lit, bright = int((want != 0).any(axis=1).sum()), int((want > 1).any(axis=1).sum())
    print("oracle: %d rays, %d casts, %d with radiance, %d with a channel above 1, %.2f s" % (
        len(want), casts, lit, bright, seconds))
    assert np.isfinite(want).all()
    assert 2 * lit >= len(want), "vacuous: %d of %d rays carry radiance" % (lit, len(want))
    assert bright >= min_bright
    return orig, dirs, keys, want, casts, seconds


def assert_same_bits(got, want, keys, what=""):
    """Every ray, every channel; the first differing ray's index, key and both values are shown."""
    got, want = np.asarray(got).reshape(-1, 3), bits(want).reshape(-1, 3)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        i = int(bad[0])
        k = "path_key(%d, 0)" % i if keys is None else "0x%08x" % (int(np.asarray(keys).view(np.uint32)[i]))
        raise AssertionError("%s: %d of %d rays differ; first ray %d, key %s: device %s (bits %s), oracle %s (bits %s)" % (
            what, len(bad), len(want), i, k, got[i].view(np.float32).tolist(), [hex(x & 0xFFFFFFFF) for x in got[i].tolist()],
            want[i].view(np.float32).tolist(), [hex(x & 0xFFFFFFFF) for x in want[i].tolist()]))


def device_radiance(r, orig, dirs, keys, src=None):
    """(the bits of r.shade_rays, rays + shadow rays the batch built).  The count comes from
    shade_rays_device into a sentinel-filled buffer, whose bits must be the wrapper's."""
    import torch
    o, d = dev(orig), dev(dirs)
    k = None if keys is None else dev(keys)
    s = None if src is None else dev(np.ascontiguousarray(src, np.int32))
    got = host(r.shade_rays(o, d, k, src=s))
    n = len(got)
    out = torch.full((n + 16, 3), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    torch.cuda.synchronize()  # (stream 0 is the renderer's own stream: not ordered after torch's fill)
    rays = r.shade_rays_device(o.data_ptr(), d.data_ptr(), n, d_key=k.data_ptr() if k is not None else 0,
                               d_src=s.data_ptr() if s is not None else 0, d_rgb=out.data_ptr())
    out = host(out)
    assert np.array_equal(out[:n], got) and (out[n:] == SENTINEL).all()
    return got, sum(rays)


def check(oracle_mod, cfg, rays=None, src=None, tuning=(), min_bright=0, device_cfg=None, what="", reference=None):
    """One case: the oracle's radiance (checked not to be vacuous), then the device's, bit for bit, and the
    rays the batch built.  The counts are the same quantity on both sides: a frame's rays + shadowRays is
    get_total_casted_rays, which equals the oracle's frame count (test_shade_rays_gpu's closed loop), and
    the oracle's counter takes a frame's camera rays as shade_rays' counter takes the given rays.
    ``reference``: oracle_radiance's result where the caller already has it."""
    import mobileraytracer_amd as m
    orig, dirs, keys, want, casts, _ = reference or oracle_radiance(oracle_mod, cfg, rays, src, min_bright)
    with m.Renderer(device_cfg or cfg) as r:
        for key, value in tuning:
            r.set_tuning(key, value)
        got, built = device_radiance(r, orig, dirs, keys, src)
        info = r.queue_info()
    assert_same_bits(got, want, keys, what)
    assert built == casts, (built, casts)
    return info


# ---- a. camera rays --------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("view", ["perspective", "orthographic"])
def test_camera_rays_are_the_oracles(oracle_mod, view, spp):
    """Origins, directions and keys bit for bit, matched by (pixel, sample).  Perspective: the water
    scene's camera file; orthographic: built-in scene 1's camera."""
    import mobileraytracer_amd as m
    cfg = config("water" if view == "perspective" else 1, PATH_TRACER, spp=spp)
    ob = oracle_of(oracle_mod, cfg)
    want = ob.camera_rays()
    ob.close()
    with m.Renderer(cfg) as r:
        got = [host(x) for x in r.camera_rays()]
    n = SIZE * SIZE * spp
    sample = np.arange(n) % spp
    order_w, order_g = np.lexsort((sample, want[3])), np.lexsort((sample, got[3]))
    assert np.array_equal(want[3][order_w], np.repeat(np.arange(SIZE * SIZE), spp))  # every pixel, spp times
    assert np.array_equal(got[3][order_g], want[3][order_w])
    assert np.array_equal(got[2][order_g], want[2].view(np.int32)[order_w])
    assert_same_bits(got[0][order_g], want[0][order_w], want[2][order_w], "origins")
    assert_same_bits(got[1][order_g], want[1][order_w], want[2][order_w], "directions")
    varying = want[0] if view == "orthographic" else want[1]
    assert len({tuple(x) for x in bits(varying).tolist()}) == n  # (every sample its own ray)


# ---- b. shaders on water ---------------------------------------------------------------------------------
@pytest.mark.parametrize("spl", [1, 2])
@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
def test_water_camera_rays(oracle_mod, shader, spl):
    check(oracle_mod, config("water", shader, spp=3, spl=spl))


@pytest.mark.parametrize("shader", [0, DEPTH_MAP, DIFFUSE, NO_SHADOWS])
def test_water_single_level_shaders(oracle_mod, tmp_path, shader):
    """k_shade_simple and k_radiance_store.  DepthMap is black beyond 1.1 |maxPoint - origin|: from the
    scene's own camera a quarter of the rays carry radiance, from the box's far lower corner all do
    (the camera of test_shade_rays_gpu's DepthMap loop)."""
    cfg = config("water", shader, spp=3)
    if shader == DEPTH_MAP:
        cam = tmp_path / "corner.cam"
        cam.write_text("t perspective\np 0.9 0.1 -0.9\nl -0.5 0.8 1.0\nu 0 1 0\nf 45 45\n")
        cfg = dataclasses.replace(cfg, camFilePath=str(cam))
    check(oracle_mod, cfg)


def test_default_keys_are_path_key_of_the_ray_index(oracle_mod):
    cfg = config("water", PATH_TRACER, spp=3)
    ob = oracle_of(oracle_mod, cfg)
    orig, dirs, keys, _ = ob.camera_rays()
    ob.close()
    check(oracle_mod, cfg, rays=(orig, dirs, None))


# ---- c. the caller's own rays ------------------------------------------------------------------------------
def water_box():
    import mobileraytracer_amd as m
    boxes = m.triangle_bvh(config("water"))[0]
    return boxes[0, :3].copy(), boxes[0, 3:].copy()


def test_callers_rays_with_radiance_above_one(oracle_mod):
    """1024 + 65 rays inside the water scene's box, a third with zero direction components and origins on
    the box's planes, random keys, PathTracer.  At least 32 of them carry a channel above 1 (oracle: 65):
    values the pixel clamp hides from every frame test."""
    n = 1024 + 65
    orig, dirs = mixed_rays(n, 11, *water_box())
    keys = np.random.default_rng(12).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    check(oracle_mod, config("water", PATH_TRACER), rays=(orig, dirs, keys), min_bright=32)


# ---- d. branching --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
def test_glassboxes_three_children_per_hit(oracle_mod, shader):
    check(oracle_mod, config("glassboxes", shader))


# ---- e. textures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
@pytest.mark.parametrize("scene", ["teapot", "corridor"])
def test_textured_scenes(oracle_mod, tmp_path, scene, shader):
    """The teapot: one textured material (seen from beside its light: from the scene's own camera a tenth
    of the PathTracer's rays carry radiance).  The corridor: two, the several-textures Kd replay."""
    if scene == "teapot":
        files = teapot_from_above(tmp_path)
    else:
        files = T.write_corridor(str(tmp_path / "corridor"), ("X", "Y"), False)[:3]
    check(oracle_mod, config(files, shader, spp=2))


# ---- f. other primitives and lights -----------------------------------------------------------------------
@pytest.mark.parametrize("scene,shader", [(0, WHITTED), (0, PATH_TRACER), (2, WHITTED), (2, PATH_TRACER), (3, WHITTED),
                                          (3, PATH_TRACER)])
def test_built_in_scenes(oracle_mod, scene, shader):
    """Planes, spheres, triangles; area lights (0, 2) and a point light (3)."""
    check(oracle_mod, config(scene, shader, spp=2))


def test_built_in_scene_without_a_light(oracle_mod):
    """Scene 1 under Whitted: spheres, an orthographic camera, no light.  Its camera sees the spheres in a
    third of the frame, so the batch is the 32 x 32 frame's camera rays that hit anything (the oracle's
    trace_rays decides) and, of those that miss, as many as keeps the hits at two thirds."""
    cfg = config(1, WHITTED, size=32)
    ob = oracle_of(oracle_mod, cfg)
    orig, dirs, keys, _ = ob.camera_rays()
    hit = ob.trace_rays(orig, dirs)[0] > 0
    ob.close()
    misses = np.flatnonzero(~hit)[: int(hit.sum()) // 2]
    keep = np.sort(np.concatenate([np.flatnonzero(hit), misses]))
    assert hit.sum() >= 128 and len(misses) >= 64
    check(oracle_mod, cfg, rays=(orig[keep], dirs[keep], keys[keep]))


# ---- g. accelerators -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("accelerator", [1, 2])
def test_naive_and_regular_grid(oracle_mod, accelerator):
    check(oracle_mod, config("water", WHITTED, spp=3, accelerator=accelerator))


# ---- h. sources ----------------------------------------------------------------------------------------------
def test_second_bounce_built_on_the_device_with_sources(oracle_mod):
    """The batch is made on the device from cast_rays' outputs: it leaves the hit points in fresh directions
    with the hits' (kind, index) as source pairs; every third ray starts just short of its hit point and
    keeps its direction, so without its source it hits the same primitive again.  Hits on lights carry no
    source and are never among the thirds (test_cast_rays_gpu's second bounce says why: the walks test
    lights without self-exclusion, the oracle's light is a Triangle that would exclude itself).  Oracle:
    650 of 1089 rays carry radiance, 254 depend on their source."""
    import torch
    import mobileraytracer_amd as m
    cfg = config("water", PATH_TRACER)
    n = 1024 + 65
    lo, hi = water_box()
    o0, d0 = mixed_rays(n, 11, lo, hi)
    fresh = mixed_rays(n, 41, lo, hi)[1]
    keys = np.random.default_rng(42).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    with m.Renderer(cfg) as r:
        o, d = dev(o0), dev(d0)
        kind, index, t = r.cast_rays(o, d)
        surface = (kind > 0) & (kind != 4)
        through = ((torch.arange(n, device="cuda") % 3 == 0) & surface).unsqueeze(1)
        tt = torch.where(through, t.unsqueeze(1) * 0.99, t.unsqueeze(1))
        o2 = torch.where((kind > 0).unsqueeze(1), o + tt * d, o)
        # (the fresh directions turned towards the box's centre: of those left as drawn, most leave the
        # scene at once and fewer than half of the rays carry radiance)
        f = dev(fresh)
        outward = ((f * (dev((lo + hi) * np.float32(0.5)) - o2)).sum(dim=1) < 0).unsqueeze(1)
        d2 = torch.where(through, d, torch.where(outward, -f, f))
        src = torch.where(surface.unsqueeze(1), torch.stack((kind, index), 1), torch.zeros((n, 2), dtype=torch.int32, device="cuda"))
        got = host(r.shade_rays(o2, d2, dev(keys), src=src.contiguous()))
        host_o2, host_d2, host_src = o2.cpu().numpy(), d2.cpu().numpy(), src.cpu().numpy()
    ob = oracle_of(oracle_mod, cfg)
    want, _ = ob.shade_rays(host_o2, host_d2, keys, host_src, threads=THREADS)
    plain, _ = ob.shade_rays(host_o2, host_d2, keys, threads=THREADS)
    ob.close()
    # (on the CPU: not vacuous, and the sources matter for these rays)
    lit, differ = int((want != 0).any(axis=1).sum()), int((bits(want) != bits(plain)).any(axis=1).sum())
    print("second bounce: %d of %d rays carry radiance, %d depend on their source" % (lit, n, differ))
    assert np.isfinite(want).all() and 2 * lit >= n and differ >= n // 20
    assert_same_bits(got, want, keys, "second bounce")


# ---- i. execution variants -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _variant_batch():
    """1024 + 65 rays: the water scene's camera rays at 4 spp and the first 65 again."""
    from oracle import oracle as O
    cfg = config("water", PATH_TRACER, spp=4)
    ob = oracle_of(O, cfg)
    orig, dirs, keys, _ = ob.camera_rays()
    ob.close()
    batch = tuple(np.concatenate([a, a[:65]]) for a in (orig, dirs, keys))
    for a in batch:
        a.setflags(write=False)
    return cfg, batch


@pytest.mark.parametrize("variant", ["resolve-then-store", "last-level-walked", "chunks", "replan"])
def test_execution_variants_keep_the_oracles_bits(oracle_mod, variant):
    """Tuning key 34 = 0: k_resolve, then k_radiance_store.  Key 7 = 0: the depth-capped level is walked.
    maxPathsPerPass 192: six chunks, the last of 129 rays (no multiple of 64).  Keys 38 = 25, 39 = 0: the
    first allocation cut to a quarter of level 1 with no slack, so a pass overflows and is replanned."""
    cfg, batch = _variant_batch()
    tuning = {"resolve-then-store": ((34, 0),), "last-level-walked": ((7, 0),), "chunks": (), "replan": ((38, 25), (39, 0))}[variant]
    chunked = variant in ("chunks", "replan")
    info = check(oracle_mod, cfg, rays=batch, tuning=tuning,
                 device_cfg=dataclasses.replace(cfg, maxPathsPerPass=192) if chunked else None, what=variant)
    print(variant, info)
    if variant == "chunks":
        assert info["replans"] == 0 and info["chunkSlots"] == 192 and info["passes"] == 6
    if variant == "replan":
        assert info["replans"] >= 1


# ---- deep trees ----------------------------------------------------------------------------------------------
def render(r, cfg):
    bm = np.full(cfg.width * cfg.height, SENTINEL, np.int32)
    r.render_frame(bm)
    return bm


def oracle_frame(oracle_mod, cfg):
    ob = oracle_of(oracle_mod, cfg)
    t0 = time.perf_counter()
    ref, rays = ob.render(np.full(cfg.width * cfg.height, SENTINEL, np.int32), threads=THREADS)
    seconds = time.perf_counter() - t0
    ob.close()
    print("oracle frame: shader %d, maxDepth %d, %d rays, %.2f s on %d threads" % (cfg.shader, cfg.maxDepth, rays, seconds,
                                                                                 THREADS))
    return ref, rays, seconds


@pytest.mark.parametrize("shader,depth", [(WHITTED, 7), (WHITTED, 10), (WHITTED, 13), (PATH_TRACER, 7), (PATH_TRACER, 10)])
def test_deep_frames_equal_the_oracle(oracle_mod, shader, depth):
    """glassboxes at maxDepth 7 .. 13 (oracle: 58,537 / 222,667 / 738,148 rays under Whitted, 317,996 /
    3,219,821 under PathTracer): the level-indexed plan, statistics and events past level 7."""
    import mobileraytracer_amd as m
    cfg = config("glassboxes", shader, depth=depth)
    ref, ref_rays, _ = oracle_frame(oracle_mod, cfg)
    with m.Renderer(cfg) as r:
        bm = render(r, cfg)
        level, q = r.frame_stats()["levelRays"], r.queue_info()
        print("levelRays", level, "queue info", q)
        assert np.array_equal(bm, ref), "%d pixels differ" % (bm != ref).sum()
        assert r.get_total_casted_rays() == ref_rays
        assert level[0] == SIZE * SIZE and all(level[lv] > 0 for lv in range(depth + 1))
        if q["passes"] == 1:  # one chunk: the last pass's totals are the frame's
            assert level[:depth + 1] == q["requestedRays"][:depth + 1]
        # (the depth-capped level's rays are counted, never written: no capacity needed)
        assert all(q["rayCap"][lv] >= q["requestedRays"][lv] for lv in range(depth))
        assert q["queueBytes"] <= q["budgetBytes"]
        bm2 = render(r, cfg)
        q2 = r.queue_info()
        print("queue info after frame 2", q2)
        assert np.array_equal(bm2, ref)
        assert q2["replansLastFrame"] == 0 and r.get_total_casted_rays() == 2 * ref_rays


def test_deepest_path_traced_frame_under_a_small_budget(oracle_mod):
    """PathTracer at maxDepth 13 under a 64 MiB queue budget (tuning key 37): 30,168,497 rays in more than
    one pass.  The oracle's frame is the cost here (about 4 s on 8 threads); where it takes more than 10 s
    the case is skipped, by the time measured."""
    import mobileraytracer_amd as m
    cfg = config("glassboxes", PATH_TRACER, depth=13)
    ref, ref_rays, seconds = oracle_frame(oracle_mod, cfg)
    if seconds > 10.0:
        pytest.skip("the oracle's frame took %.1f s on this machine" % seconds)
    with m.Renderer(cfg) as r:
        r.set_tuning(37, 64)
        bm = render(r, cfg)
        level, q = r.frame_stats()["levelRays"], r.queue_info()
        print("levelRays", level, "queue info", q)
        assert np.array_equal(bm, ref), "%d pixels differ" % (bm != ref).sum()
        assert r.get_total_casted_rays() == ref_rays
        assert all(level[lv] > 0 for lv in range(14))
        assert q["budgetBytes"] == 64 << 20 and q["queueBytes"] <= q["budgetBytes"] and q["passes"] > 1


@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
@pytest.mark.parametrize("depth", [7, 10, 13])
def test_deep_float_radiance(oracle_mod, shader, depth):
    """64 camera rays of glassboxes (every fourth pixel) at maxDepth 7, 10 and 13.  The deepest level
    matters at float precision: the oracle's radiance at maxDepth differs in bits from its radiance at
    maxDepth - 1 for at least a quarter of the rays (measured: all 64, every depth and shader)."""
    cfg = config("glassboxes", shader, depth=depth)
    ob = oracle_of(oracle_mod, cfg)
    orig, dirs, keys, _ = ob.camera_rays()
    ob.close()
    rays = tuple(a[::4] for a in (orig, dirs, keys))
    shallower = oracle_radiance(oracle_mod, dataclasses.replace(cfg, maxDepth=depth - 1), rays)
    want = oracle_radiance(oracle_mod, cfg, rays)
    differ = int((bits(want[3]) != bits(shallower[3])).any(axis=1).sum())
    print("maxDepth %d against %d: %d of 64 rays differ in bits; the oracle's share %.2f s" % (
        depth, depth - 1, differ, want[5] + shallower[5]))
    assert 4 * differ >= 64
    check(oracle_mod, cfg, reference=want)


def test_deep_float_radiance_on_water(oracle_mod):
    """PathTracer at maxDepth 13 on the water scene: cheap, since Russian roulette ends most paths early -
    which also means the last level reaches few rays (oracle: 3 of 256 differ from maxDepth 12), so the
    quarter asked of glassboxes cannot hold here; at least one ray must reach it."""
    cfg = config("water", PATH_TRACER, depth=13)
    shallower = oracle_radiance(oracle_mod, dataclasses.replace(cfg, maxDepth=12))
    want = oracle_radiance(oracle_mod, cfg)
    differ = int((bits(want[3]) != bits(shallower[3])).any(axis=1).sum())
    print("water, maxDepth 13 against 12: %d of 256 rays differ in bits" % differ)
    assert differ >= 1
    check(oracle_mod, cfg, reference=want)


def test_the_depth_limit(oracle_mod):
    """maxDepth 13 constructs and renders, 14 is refused (maxDepth + 2 levels of 16), 0 means 6."""
    import mobileraytracer_amd as m
    cfg = config(0, WHITTED, depth=13)
    ref, ref_rays, _ = oracle_frame(oracle_mod, cfg)
    with m.Renderer(cfg) as r:
        assert np.array_equal(render(r, cfg), ref) and r.get_total_casted_rays() == ref_rays
    with pytest.raises(RuntimeError, match="maxDepth too large"):
        m.Renderer(config(0, WHITTED, depth=14))
    six, six_rays, _ = oracle_frame(oracle_mod, config("glassboxes", WHITTED, depth=6))
    five, five_rays, _ = oracle_frame(oracle_mod, config("glassboxes", WHITTED, depth=5))
    assert not np.array_equal(six, five) and six_rays > five_rays  # (the depth shows in this frame)
    cfg = config("glassboxes", WHITTED, depth=0)
    with m.Renderer(cfg) as r:
        assert np.array_equal(render(r, cfg), six) and r.get_total_casted_rays() == six_rays
