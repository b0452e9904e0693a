"""Ray queries (mrt_cast_rays_device): caller-supplied rays, resident in device memory, through the
renderer's walks.  The contract is bit-equality with the CPU oracle's trace_rays (and with the
host-array diagnostic mrt_trace_rays), so every check here is exact: kind, input index, the bits of
t, the occlusion flags.

Outputs start filled with a sentinel where it matters, so an entry written out of place, or not
written at all, shows up.
"""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0x12345678  # (as int32 and as the bits of a float32: 5.69e-28, no t the walks produce)
WHITTED = 1
UP = (0.0, 1.0, 0.0)


def bits(t):
    return np.ascontiguousarray(t, np.float32).view(np.int32)


def same_hits(got, ref):
    """(kind, index, t) triples equal, t by its bits."""
    return (np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
            and np.array_equal(bits(got[2]), bits(ref[2])))


def water_cfg():
    """tests/golden/CornellBox (Water) at 16 x 16, 1 spp: the smallest level-1 queue a frame allows."""
    import mobileraytracer_amd as m
    from mobileraytracer_amd import scenes
    obj, mtl, cam = scenes.cornell_water()
    return m.Config(width=16, height=16, shader=WHITTED, sceneIndex=-1, objFilePath=obj, mtlFilePath=mtl,
                    camFilePath=cam)


def oracle_of(oracle_mod, cfg):
    return oracle_mod.Oracle(cfg.width, cfg.height, cfg.shader, cfg.sceneIndex, cfg.samplesPixel, cfg.samplesLight,
                             cfg.maxDepth, obj=cfg.objFilePath, mtl=cfg.mtlFilePath, cam=cfg.camFilePath,
                             accelerator=cfg.accelerator)


def mixed_rays(n, seed, lo, hi):
    """A fixed-seed mix.  Two thirds: origins uniform in the box [lo, hi], directions normal.  One
    third: one or two direction components exactly 0 (1/d infinite: the reference-tree path) and the
    origins exactly on a plane of the box.  Shuffled, so every chunk and wave holds both kinds."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    special = rng.permutation(n)[: n // 3]
    for j, i in enumerate(special):
        axes = rng.permutation(3)
        d[i, axes[: 1 + j % 2]] = 0.0                      # one zero component, or two (axis-aligned)
        a = rng.integers(0, 3)
        o[i, a] = (lo, hi)[rng.integers(0, 2)][a]          # exactly on a box plane
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    assert ((d[special] == 0).sum(axis=1) >= 1).all()
    return o, d


def dists(n, seed):
    return np.random.default_rng(seed).uniform(0.05, 3.0, n).astype(np.float32)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared references are read-only)


def cast(r, o, d, dist=None, src=None, any_hit=False):
    """Renderer.cast_rays on host arrays (uploaded here), the results back as numpy arrays."""
    res = r.cast_rays(dev(o), dev(d), dist=None if dist is None else dev(dist),
                      src=None if src is None else dev(src), any_hit=any_hit)
    return res.cpu().numpy() if any_hit else tuple(x.cpu().numpy() for x in res)


@pytest.fixture(scope="module")
def water(oracle_mod):
    """Case 1's rays and the oracle's answers, computed once and shared (read-only): closest hit for
    n = 3 cap + 65 rays of the level-1 ray queue's capacity, any hit for 3 shadowCap + 65: at least
    four chunks each, the last one partial and no multiple of 64."""
    import mobileraytracer_amd as m
    cfg = water_cfg()
    with m.Renderer(cfg) as r:
        q = r.queue_info()
    cap, shadow_cap = q["rayCap"][0], q["shadowCap"][0]
    assert cap >= 64 and shadow_cap >= 64
    boxes, _, _, _ = m.triangle_bvh(cfg)
    lo, hi = boxes[0, :3].copy(), boxes[0, 3:].copy()
    w = {"cfg": cfg, "lo": lo, "hi": hi, "cap": cap, "shadowCap": shadow_cap}
    w["o"], w["d"] = mixed_rays(3 * cap + 65, 11, lo, hi)
    w["ao"], w["ad"] = mixed_rays(3 * shadow_cap + 65, 12, lo, hi)
    w["dist"] = dists(len(w["ao"]), 13)
    ob = oracle_of(oracle_mod, cfg)
    w["hits"] = ob.trace_rays(w["o"], w["d"])
    w["occ"] = ob.trace_rays(w["ao"], w["ad"], dist=w["dist"], any_hit=True)[0]
    ob.close()
    # (on the CPU, before any comparison: an all-miss or all-clear batch must not pass vacuously)
    hit, occluded = float((w["hits"][0] > 0).mean()), float(w["occ"].mean())
    print("water rays: cap %d shadowCap %d, oracle hit fraction %.3f, occluded %.3f" % (cap, shadow_cap, hit, occluded))
    assert 0.2 < hit < 0.98 and 0.02 < occluded < 0.98
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w


# ---- 1. oracle parity, triangles ---------------------------------------------------------------------
def test_chunked_batches_equal_the_oracle_and_the_host_path(water):
    import mobileraytracer_amd as m
    with m.Renderer(water["cfg"]) as r:
        bytes0 = r.scene_info()["deviceBytes"]
        got = cast(r, water["o"], water["d"])
        bytes1 = r.scene_info()["deviceBytes"]
        occ = cast(r, water["ao"], water["ad"], dist=water["dist"], any_hit=True)
        host = r.trace_rays(water["o"], water["d"])
        host_occ = r.trace_rays(water["ao"], water["ad"], dist=water["dist"], any_hit=True)[0]
        q = r.queue_info()
        assert (q["rayCap"][0], q["shadowCap"][0]) == (water["cap"], water["shadowCap"])  # the chunking assumed
        # the tables are made at the first query, counted from then on, and made once
        n_prims = sum(r.scene_info()[k] for k in ("triangles", "planes", "spheres"))
        assert bytes1 - bytes0 >= 4 * n_prims and r.scene_info()["deviceBytes"] == bytes1
        assert r.get_total_casted_rays() == 0
    assert same_hits(got, water["hits"])
    assert np.array_equal(occ, water["occ"])
    assert same_hits(got, host) and np.array_equal(occ, host_occ)


# ---- 2. planes, spheres and area lights --------------------------------------------------------------
# built-in scenes: 3 spheres2_Scene (a plane, five spheres), 2 cornellBox2_Scene (six planes, two
# spheres, two triangles, and two area lights: the ceiling quad |x|, |z| < 0.25 at y = 0.99)
@pytest.mark.parametrize("scene,kinds", [(3, (1, 2)), (2, (1, 2, 4))])
def test_planes_spheres_and_lights(oracle_mod, scene, kinds):
    import mobileraytracer_amd as m
    cfg = m.Config(width=16, height=16, shader=WHITTED, sceneIndex=scene)
    n = 257
    o, d = mixed_rays(n, 20 + scene, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    if 4 in kinds:  # the first 32 rays aimed at the light quad, which uniform directions seldom find
        rng = np.random.default_rng(40)
        aim = np.stack([rng.uniform(-0.25, 0.25, 32), np.full(32, 0.99), rng.uniform(-0.25, 0.25, 32)], 1) - o[:32]
        d[:32] = (aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(np.float32)
    dist = dists(n, 30 + scene)
    ob = oracle_of(oracle_mod, cfg)
    ref = ob.trace_rays(o, d)
    ref_occ = ob.trace_rays(o, d, dist=dist, any_hit=True)[0]
    ob.close()
    for k in kinds:
        assert (ref[0] == k).sum() >= 4, "the oracle hits too few primitives of kind %d" % k
    assert 0.02 < ref_occ.mean() < 0.98
    with m.Renderer(cfg) as r:
        info = r.scene_info()
        if 1 in kinds:
            assert info["planes"] > 0 and info["spheres"] > 0
        if 4 in kinds:
            assert info["lights"] > 0
        got = cast(r, o, d)
        occ = cast(r, o, d, dist=dist, any_hit=True)
        host = r.trace_rays(o, d)
    assert same_hits(got, ref) and same_hits(got, host)
    assert np.array_equal(occ, ref_occ)


# ---- 3. small and odd sizes --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches_write_their_entries_and_nothing_else(water, n):
    import torch
    import mobileraytracer_amd as m
    o, d, dist = dev(water["o"][:n]), dev(water["d"][:n]), dev(water["dist"][:n])
    ao, ad = dev(water["ao"][:n]), dev(water["ad"][:n])
    ref = tuple(x[:n] for x in water["hits"])

    def outputs():
        return (torch.full((n + 64,), SENTINEL, dtype=torch.int32, device="cuda"),
                torch.full((n + 64,), SENTINEL, dtype=torch.int32, device="cuda"),
                torch.full((n + 64,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32))

    def host(x):
        return x.view(torch.int32).cpu().numpy()

    with m.Renderer(water["cfg"]) as r:
        k, i, t = outputs()
        k2, i2, t2 = outputs()
        _, i3, t3 = outputs()
        k4, i4, t4 = outputs()
        torch.cuda.synchronize()  # (stream 0 is the renderer's own stream: not ordered after torch's fills)
        r.cast_rays_device(o.data_ptr(), d.data_ptr(), n, d_kind=k.data_ptr(), d_index=i.data_ptr(), d_t=t.data_ptr())
        # d_index and d_t not wanted: only kind is written
        r.cast_rays_device(o.data_ptr(), d.data_ptr(), n, d_kind=k2.data_ptr())
        # each output alone
        r.cast_rays_device(o.data_ptr(), d.data_ptr(), n, d_index=i3.data_ptr())
        r.cast_rays_device(o.data_ptr(), d.data_ptr(), n, d_t=t3.data_ptr())
        # any hit: d_index / d_t untouched even when given
        r.cast_rays_device(ao.data_ptr(), ad.data_ptr(), n, d_dist=dist.data_ptr(), any_hit=True, d_kind=k4.data_ptr(),
                           d_index=i4.data_ptr(), d_t=t4.data_ptr())
        torch.cuda.synchronize()
    for kk, ii, tt in ((k, i, t), (k2, None, None), (None, i3, t3)):
        for x, want in ((kk, ref[0]), (ii, ref[1]), (tt, bits(ref[2]))):
            if x is not None:
                assert np.array_equal(host(x)[:n], want) and (host(x)[n:] == SENTINEL).all()
    assert (host(i2) == SENTINEL).all() and (host(t2) == SENTINEL).all()
    assert np.array_equal(host(k4)[:n], water["occ"][:n]) and (host(k4)[n:] == SENTINEL).all()
    assert (host(i4) == SENTINEL).all() and (host(t4) == SENTINEL).all()


# ---- 4. strides --------------------------------------------------------------------------------------
def test_strided_rays_give_the_packed_results(water):
    import torch
    import mobileraytracer_amd as m
    n = water["cap"] + 65  # two chunks: the stride is applied to the batch's ray index, not the chunk's
    o, d = water["o"][:n], water["d"][:n]
    ref = tuple(x[:n] for x in water["hits"])
    od = dev(np.concatenate([o, d], axis=1))                                       # (n, 6): origin | direction
    pad = np.float32(np.nan)
    o4 = dev(np.concatenate([o, np.full((n, 1), pad, np.float32)], axis=1))        # (n, 4), padded
    d4 = dev(np.concatenate([d, np.full((n, 1), pad, np.float32)], axis=1))
    with m.Renderer(water["cfg"]) as r:
        k = torch.empty(n, dtype=torch.int32, device="cuda")
        i = torch.empty(n, dtype=torch.int32, device="cuda")
        t = torch.empty(n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (stream 0 is the renderer's own stream: not ordered after torch's uploads)
        r.cast_rays_device(od.data_ptr(), od.data_ptr() + 12, n, orig_stride=6, dir_stride=6, d_kind=k.data_ptr(),
                           d_index=i.data_ptr(), d_t=t.data_ptr())
        torch.cuda.synchronize()
        six = (k.cpu().numpy(), i.cpu().numpy(), t.cpu().numpy())
        four = tuple(x.cpu().numpy() for x in r.cast_rays(o4[:, :3], d4[:, :3]))   # strides from the tensors
        views = tuple(x.cpu().numpy() for x in r.cast_rays(od[:, :3], od[:, 3:]))
        occ = r.cast_rays(od[:, :3], od[:, 3:], dist=dev(water["dist"][:n]), any_hit=True).cpu().numpy()
        occ_packed = cast(r, o, d, dist=water["dist"][:n], any_hit=True)
    assert same_hits(six, ref) and same_hits(four, ref) and same_hits(views, ref)
    assert np.array_equal(occ, occ_packed)


# ---- 5. device-side chaining with sources ------------------------------------------------------------
def test_second_bounce_built_on_the_device_with_sources(oracle_mod, water):
    """Batch B is made on the device from batch A's outputs: it leaves A's hit points in fresh
    directions, with A's (kind, index) as the source pairs.  A third of B starts just short of the
    hit point and keeps A's direction: without its source pair such a ray hits A's primitive again,
    with it it passes through, so a source that is dropped or mapped wrongly shows.  (Not where A
    hit a light: the walks test lights without self-exclusion, since no ray of the reference leaves
    one, while the oracle's light is a Triangle that would exclude itself.  Those rays leave the hit
    point itself in a fresh direction, like the other two thirds.)"""
    import torch
    import mobileraytracer_amd as m
    n = 2 * water["cap"] + 65
    fresh = mixed_rays(n, 41, water["lo"], water["hi"])[1]
    with m.Renderer(water["cfg"]) as r:
        o, d = dev(water["o"][:n]), dev(water["d"][:n])
        kind, index, t = r.cast_rays(o, d)
        hit = (kind > 0).unsqueeze(1)
        through = ((torch.arange(n, device="cuda") % 3 == 0) & (kind != 4)).unsqueeze(1)
        tt = torch.where(through, t.unsqueeze(1) * 0.99, t.unsqueeze(1))
        o2 = torch.where(hit, o + tt * d, o)
        d2 = torch.where(through, d, dev(fresh))
        src = torch.stack((kind, index), 1)
        got = tuple(x.cpu().numpy() for x in r.cast_rays(o2, d2, src=src))
        # every pair corrupted: a kind that is none, an index at / past the count, a negative one
        counts = {1: r.scene_info()["planes"], 2: r.scene_info()["spheres"], 3: r.scene_info()["triangles"],
                  4: r.scene_info()["lights"]}
        bad = src.cpu().numpy().copy()
        lane = np.arange(n) % 4
        bad[lane == 0, 0] = 9
        bad[lane == 1, 0], bad[lane == 1, 1] = 3, counts[3] + np.arange((lane == 1).sum()) * 1000003 % (1 << 30)
        bad[lane == 2, 0], bad[lane == 2, 1] = 1 + np.arange((lane == 2).sum()) % 4, -1 - np.arange((lane == 2).sum())
        bad[lane == 3, 0], bad[lane == 3, 1] = -3, 0
        bad[5, :] = (3, -(1 << 31))
        bad[6, :] = (4, counts[4])
        bad[7, :] = (2, counts[2])
        got_bad = tuple(x.cpu().numpy() for x in r.cast_rays(o2, d2, src=dev(bad)))
        got_none = tuple(x.cpu().numpy() for x in r.cast_rays(o2, d2))
        host_o2, host_d2, host_src = o2.cpu().numpy(), d2.cpu().numpy(), src.cpu().numpy()
    assert np.array_equal(host_src[:, 0], water["hits"][0][:n]) and np.array_equal(host_src[:, 1], water["hits"][1][:n])
    ob = oracle_of(oracle_mod, water["cfg"])
    ref = ob.trace_rays(host_o2, host_d2, src=host_src)
    ref_none = ob.trace_rays(host_o2, host_d2)
    ob.close()
    # (on the CPU: the sources matter for these rays)
    differ = int(((ref[0] != ref_none[0]) | (ref[1] != ref_none[1])).sum())
    print("second bounce: %d of %d rays depend on their source" % (differ, n))
    assert differ >= n // 20
    assert same_hits(got, ref)
    assert same_hits(got_none, ref_none) and same_hits(got_bad, got_none)


# ---- 6. walk and cull settings -----------------------------------------------------------------------
@pytest.mark.parametrize("tuning", [((1, 0),), ((2, 0),), ((2, 3),), ((28, 1),), ((1, 0), (28, 1))])
def test_walk_and_cull_settings_give_identical_results(water, tuning):
    import mobileraytracer_amd as m
    with m.Renderer(water["cfg"]) as r:
        for key, value in tuning:
            r.set_tuning(key, value)
        got = cast(r, water["o"], water["d"])
        n = 2 * water["cap"] + 65
        occ = cast(r, water["ao"][:n], water["ad"][:n], dist=water["dist"][:n], any_hit=True)
    assert same_hits(got, water["hits"])
    assert np.array_equal(occ, water["occ"][:n])


# ---- 7. frames are undisturbed -----------------------------------------------------------------------
def test_frames_between_queries_keep_their_bits_and_counts(oracle_mod):
    import mobileraytracer_amd as m
    from mobileraytracer_amd import scenes
    obj, mtl, cam = scenes.glass_boxes()
    cfg = m.Config(width=64, height=48, shader=WHITTED, samplesPixel=1, samplesLight=1, maxDepth=4, sceneIndex=-1,
                   objFilePath=obj, mtlFilePath=mtl, camFilePath=cam)
    boxes, _, _, _ = m.triangle_bvh(cfg)
    n = 1000
    o, d = mixed_rays(n, 51, boxes[0, :3], boxes[0, 3:])
    dist = dists(n, 52)
    ob = oracle_of(oracle_mod, cfg)
    ref = ob.trace_rays(o, d)
    ref_occ = ob.trace_rays(o, d, dist=dist, any_hit=True)[0]
    ob.close()
    assert 0.2 < (ref[0] > 0).mean() and 0.02 < ref_occ.mean() < 0.98
    cams = [(0, (-0.25, 0.125, 0.5), (0.0, 0.0, -1.0), UP, 60.0, 60.0),
            (0, (0.375, -0.25, 0.25), (0.5, 0.25, -1.0), UP, 50.0, 45.0)]
    frames, queries = [], []

    def frame(r):
        before = r.get_total_casted_rays()
        bm = np.full(64 * 48, SENTINEL, np.int32)
        r.render_frame(bm)
        st = r.frame_stats()
        frames.append((bm, (st["rays"], st["shadowRays"], st["primaryRays"], tuple(st["levelRays"]),
                            tuple(st["levelShadowRays"])), r.get_total_casted_rays() - before))

    def query(r, any_hit):
        before, st = r.get_total_casted_rays(), r.frame_stats()
        queries.append(cast(r, o, d, dist=dist, any_hit=True) if any_hit else cast(r, o, d))
        now = r.frame_stats()
        assert r.get_total_casted_rays() == before
        assert all(now[k] == st[k] for k in st if not k.endswith("Ms"))  # (a query is no frame)

    with m.Renderer(cfg) as r:
        frame(r)
        query(r, False)
        frame(r)
        query(r, True)
        slots0 = r.queue_info()["chunkSlots"]
        views = np.full((2, 64 * 48), SENTINEL, np.int32)
        r.render_views(cams, views)
        assert r.queue_info()["chunkSlots"] != slots0  # the plan was re-made for the batch's slot count
        query(r, False)
        query(r, True)
        frame(r)
    assert not (frames[0][0] == SENTINEL).all() and frames[0][2] > 0
    for bm, counts, rays in frames[1:]:
        assert np.array_equal(bm, frames[0][0]) and counts == frames[0][1] and rays == frames[0][2]
    assert same_hits(queries[0], ref) and same_hits(queries[2], ref)
    assert np.array_equal(queries[1], ref_occ) and np.array_equal(queries[3], ref_occ)


# ---- 8. the caller's stream --------------------------------------------------------------------------
def test_query_is_ordered_on_the_callers_stream(water):
    """On a stream of the caller's: a long run of kernels, then the kernels that fill the ray tensors,
    then the query, then reductions of its outputs - and no synchronisation before the final copies.
    A query that started before the fill would read zeros, a reduction that started before the query
    the sentinel."""
    import torch
    import mobileraytracer_amd as m
    n = len(water["o"])
    src_o, src_d = dev(water["o"]), dev(water["d"])
    want = [dev(x) for x in (water["hits"][0], water["hits"][1], bits(water["hits"][2]))]
    busy = torch.ones(1 << 24, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with m.Renderer(water["cfg"]) as r:
        with torch.cuda.stream(stream):
            o = torch.zeros(n, 3, device="cuda")
            d = torch.zeros(n, 3, device="cuda")
            k = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
            i = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
            t = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
            for _ in range(200):
                busy.mul_(1.0001)
            o.add_(src_o)
            d.add_(src_d)
            r.cast_rays_device(o.data_ptr(), d.data_ptr(), n, d_kind=k.data_ptr(), d_index=i.data_ptr(), d_t=t.data_ptr(),
                               stream=stream.cuda_stream)
            wrong = (k != want[0]).sum() + (i != want[1]).sum() + (t.view(torch.int32) != want[2]).sum()
            hits = (k > 0).sum()
            wrong, hits = int(wrong.cpu()), int(hits.cpu())  # (the first wait for the device)
    assert wrong == 0 and hits == int((water["hits"][0] > 0).sum())


# ---- 9. device groups are refused --------------------------------------------------------------------
def test_device_group_refuses_a_query():
    import torch
    import mobileraytracer_amd as m
    cfg = m.Config(width=64, height=48, shader=WHITTED, sceneIndex=0)
    with m.Renderer(cfg) as r:
        want = np.full(64 * 48, SENTINEL, np.int32)
        r.render_frame(want)
        rays = r.get_total_casted_rays()
    o, d = (dev(x) for x in mixed_rays(64, 61, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)))
    k = torch.full((64,), SENTINEL, dtype=torch.int32, device="cuda")
    with m.Renderer(dataclasses.replace(cfg, devices=[0, 0])) as g:
        with pytest.raises(RuntimeError, match="device groups are not supported"):
            g.cast_rays_device(o.data_ptr(), d.data_ptr(), 64, d_kind=k.data_ptr())
        with pytest.raises(RuntimeError, match="device groups are not supported"):
            g.cast_rays(o, d)
        torch.cuda.synchronize()
        assert (k.cpu().numpy() == SENTINEL).all() and g.get_total_casted_rays() == 0
        bm = np.full(64 * 48, SENTINEL, np.int32)
        g.render_frame(bm)
        assert np.array_equal(bm, want) and g.get_total_casted_rays() == rays


# ---- 10. the torch wrapper never forwards a layout the entry point would misread --------------------
def test_broadcast_and_odd_layouts_give_the_packed_results(water):
    """A stride of 0 means 'packed' to the C entry point, so an expanded tensor (all rays from one
    point: rows 0 floats apart) must not reach it as it is.  One origin expanded over n rays, one
    direction expanded over n origins, and column-major tensors equal the same rays packed; n spans
    two chunks, so a stride misread as 3 would read far past the 12-byte origin."""
    import torch
    import mobileraytracer_amd as m
    n = water["cap"] + 65
    o, d = dev(water["o"][:n]), dev(water["d"][:n])
    one_o, one_d = o[7:8], d[9:10]
    with m.Renderer(water["cfg"]) as r:
        fan = r.cast_rays(one_o.expand(n, 3), d)
        fan_packed = r.cast_rays(one_o.repeat(n, 1), d)
        beam = r.cast_rays(o, one_d.expand(n, 3))
        beam_packed = r.cast_rays(o, one_d.repeat(n, 1))
        assert one_o.expand(n, 3).stride() == (0, 1)  # the layout meant
        column_major = r.cast_rays(o.t().contiguous().t(), d.t().contiguous().t())
        occ = r.cast_rays(one_o.expand(n, 3), d, dist=dev(water["dist"][:n]), any_hit=True)
        occ_packed = r.cast_rays(one_o.repeat(n, 1), d, dist=dev(water["dist"][:n]), any_hit=True)
        single = r.cast_rays(one_o, one_d)  # n = 1: any row stride
        res = [tuple(x.cpu().numpy() for x in y) for y in (fan, fan_packed, beam, beam_packed, column_major, single)]
        occ, occ_packed = occ.cpu().numpy(), occ_packed.cpu().numpy()
    assert same_hits(res[0], res[1]) and same_hits(res[2], res[3])
    assert (res[1][0] > 0).any() and (res[3][0] > 0).any()
    assert same_hits(res[4], tuple(x[:n] for x in water["hits"]))
    assert np.array_equal(occ, occ_packed) and 0 < occ.sum() < n
    assert all(len(x) == 1 for x in res[5])


def test_wrapper_refuses_tensors_it_cannot_hand_to_the_device(water):
    import torch
    import mobileraytracer_amd as m
    n = 64
    o, d = dev(water["o"][:n]), dev(water["d"][:n])
    dist, src = dev(water["dist"][:n]), torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    with m.Renderer(water["cfg"]) as r:
        for args, kw in (((o.cpu(), d), {}), ((o, d.cpu()), {}), ((o, d), dict(dist=dist.cpu(), any_hit=True)),
                         ((o, d), dict(src=src.cpu())), ((o.double(), d), {}), ((o, d[:, :2]), {}), ((o, d[:32]), {}),
                         ((o[:, 0], d), {}), ((o, d), dict(dist=dist[:32], any_hit=True)), ((o, d), dict(src=src[:, :1])),
                         ((o, d), dict(any_hit=True))):
            with pytest.raises(ValueError):
                r.cast_rays(*args, **kw)
        # an empty batch (device-side chaining with no hits left): empty results, no call
        kind, index, t = r.cast_rays(o[:0], d[:0], src=src[:0])
        assert (kind.shape, index.shape, t.shape) == ((0,), (0,), (0,)) and kind.is_cuda
        assert (kind.dtype, index.dtype, t.dtype) == (torch.int32, torch.int32, torch.float32)
        assert r.cast_rays(o[:0], d[:0], dist=dist[:0], any_hit=True).shape == (0,)
        assert r.scene_info()["deviceBytes"] > 0 and same_hits(
            tuple(x.cpu().numpy() for x in r.cast_rays(o, d)), tuple(x[:n] for x in water["hits"]))
