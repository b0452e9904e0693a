"""What a triangle list alone decides about the walks (tests/shape_scenes.py): the depth of the tree
(the packet walk's stack limit of 128 entries, the per-lane walks' spill stacks), zero-area triangles
in the leaves of real ones, boxes that are not finite (no quantized walk tree: every ray walks the
reference tree) and an outlier that stretches the 16-bit grid over 2^40.

The CPU half checks that the scenes are what they claim (on the oracle alone), that the host build
equals the oracle's on them, the walk tree's containment and the stack need.  The GPU half compares
primary hits, Whitted and PathTracer frames, ray counts and random rays with the oracle, bit for
bit, and the walk and cull settings with each other.  No tolerance anywhere.
"""
import dataclasses
import functools
import os

import numpy as np
import pytest

import shape_scenes as S
from test_golden_cpu import _bvh_walk
from test_views_gpu import sentinel
from test_walk_tree_cpu import check_walk_tree_holds_reference_leaves

WHITTED, PATH_TRACER = 1, 2
SIZE, MAX_DEPTH = 64, 3
PACKET_STACK = 128  # kPacketStack (mrt_kernels.hpp)
STACKS = ["stack%d" % n for n in S.STACK_CASES]
DEEP = "stack%d" % S.STACK_DEEP
ALL = STACKS + list(S.SCENES)
QUANTIZED = [n for n in ALL if n not in S.NON_FINITE]
# two cameras of the .cam text's form (position, lookAt, (f.u, f.v)); the first is the scenes' own
CAMS = [((0.0, 0.0, -10.0), (0.0, 0.0, 0.0), (60.0, 60.0)), ((1.5, 0.5, -9.0), (0.25, 0.0, 0.0), (50.0, 50.0))]


class Shape:
    """One generated scene: its files, its configurations and the oracle's answers, each computed at
    most once and shared read-only."""

    def __init__(self, path, name):
        self.name = name
        self.obj, self.mtl, self.cam, self.first = S.write_scene(path, name)

    def cfg(self, shader=WHITTED, spp=1, **kw):
        import mobileraytracer_amd as m
        return m.Config(width=SIZE, height=SIZE, shader=shader, samplesPixel=spp, samplesLight=1, maxDepth=MAX_DEPTH,
                        sceneIndex=-1, objFilePath=self.obj, mtlFilePath=self.mtl, camFilePath=self.cam, **kw)

    def oracle(self, shader=WHITTED, spp=1):
        from oracle import oracle as O
        return O.Oracle(SIZE, SIZE, shader, -1, spp, 1, MAX_DEPTH, obj=self.obj, mtl=self.mtl, cam=self.cam)

    @functools.lru_cache(maxsize=None)
    def bvh(self):
        o = self.oracle()
        out = o.triangle_bvh() + (o.counts()["triangles"],)
        o.close()
        return out

    @functools.lru_cache(maxsize=None)
    def hits(self):
        o = self.oracle()
        out = o.primary_hits()
        o.close()
        for a in out:
            a.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def frame(self, shader, spp):
        """(bitmap, casted rays) of the oracle from a sentinel-filled bitmap."""
        o = self.oracle(shader, spp)
        bm = sentinel(SIZE * SIZE)
        _, rays = o.render(bm, threads=min(16, os.cpu_count() or 1))
        o.close()
        bm.setflags(write=False)
        return bm, rays

    @functools.lru_cache(maxsize=None)
    def rays(self):
        """The recipe of test_regular_grid_random_rays around the BASE scene's box (never the scene's
        own, which may not be finite): origins, directions, distances and the oracle's closest hits
        and occlusion flags."""
        lo, hi = np.array(S.BASE_LO), np.array(S.BASE_HI)
        rng = np.random.default_rng(11)
        n = 20000
        o = (lo - 0.25 * (hi - lo) + rng.random((n, 3)) * 1.5 * (hi - lo)).astype(np.float32)
        d = rng.normal(size=(n, 3))
        d[: n // 10, rng.integers(0, 3)] = 0.0  # axis-parallel directions: 1/d infinite, the reference tree
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        dist = (rng.random(n) * np.linalg.norm(hi - lo)).astype(np.float32)
        ob = self.oracle()
        hit = ob.trace_rays(o, d)
        occ = ob.trace_rays(o, d, dist=dist, any_hit=True)[0]
        ob.close()
        for a in (o, d, dist, occ) + tuple(hit):
            a.setflags(write=False)
        return o, d, dist, hit, occ


@pytest.fixture(scope="module")
def shapes(oracle_mod, tmp_path_factory):
    root = tmp_path_factory.mktemp("shapes")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Shape(str(root / name), name)
        return cache[name]
    return get


def depth_of(off, cnt):
    """Levels of a BVHNode array (a lone leaf: 1)."""
    best, st = 0, [(0, 1)]
    while st:
        i, d = st.pop()
        best = max(best, d)
        if cnt[i] == 0 and len(cnt) > 1:
            st += [(int(off[i]), d + 1), (int(off[i]) + 1, d + 1)]
    return best


def bits(t):
    return np.ascontiguousarray(t, np.float32).view(np.int32)


def same_hits(got, ref):
    """(kind, index, t) triples equal, t by its bits.  Where the reference's t is NaN - a ray whose last
    accepted length was a non-finite triangle's, a miss - any NaN is the same answer: the sign and the
    payload of a NaN are the processor's (x86's default NaN has the sign bit set, the GPU's has not)."""
    t, rt = np.ascontiguousarray(got[2], np.float32), np.ascontiguousarray(ref[2], np.float32)
    nan = np.isnan(rt)
    return (np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
            and np.array_equal(np.isnan(t), nan) and np.array_equal(bits(t)[~nan], bits(rt)[~nan]))


# ---- CPU 1: the scenes are what they claim (the oracle alone) -----------------------------------------
@pytest.mark.parametrize("n", list(S.STACK_CASES))
def test_stack_depths_are_the_recorded_ones(shapes, n):
    """The reference tree of stack(n) has the depth written beside the case (one split peels one
    coincident copy off); the deep case lies between 400 and 500, every case below the reference's
    own stack of 512."""
    _, off, cnt, _, ntri = shapes("stack%d" % n).bvh()
    depth = depth_of(off, cnt)
    print("stack(%d): %d triangles, reference depth %d" % (n, ntri, depth))
    assert depth == S.STACK_CASES[n][0]
    assert depth < 512
    if n == S.STACK_DEEP:
        assert 400 <= depth <= 500


def test_degenerate_leaves_mix_zero_area_and_real_triangles(shapes):
    s = shapes("degenerate")
    _, off, cnt, order, ntri = s.bvh()
    assert ntri - s.first >= 50
    mixed = 0
    for i in range(len(cnt)):
        if cnt[i] > 0:
            zero = int((order[off[i]:off[i] + cnt[i]] >= s.first).sum())
            mixed += 0 < zero < cnt[i]
    print("degenerate: %d of %d leaves hold a zero-area and a real triangle" % (mixed, int((cnt > 0).sum())))
    assert mixed >= 8
    kind, index, _ = s.hits()
    assert not ((kind == 3) & (index >= s.first)).any()  # Moller-Trumbore rejects them at |det| < eps


@pytest.mark.parametrize("name", S.NON_FINITE)
def test_non_finite_scenes_change_the_references_answer(shapes, name):
    """The root box has a non-finite component, and the reference's own primary hits differ from the
    plain base scene's on ordinary pixels: a product that quietly walked a tree of its own would show."""
    s = shapes(name)
    boxes = s.bvh()[0]
    assert not np.isfinite(boxes[0]).all(), boxes[0]
    base = shapes("base").hits()
    mine = s.hits()
    differ = float(((mine[0] != base[0]) | (mine[1] != base[1]) | (bits(mine[2]) != bits(base[2]))).mean())
    print("%s: root box %s, %.1f %% of the primary hits differ from the base scene's" % (name, boxes[0], 100 * differ))
    assert differ >= 0.05
    # how they differ: the non-finite triangle's test returns a NaN t, which Triangle.cpp:104 accepts
    # and Shader.cpp:122 turns into a miss when nothing is accepted after it
    nan = np.isnan(mine[2])
    assert nan.mean() >= 0.05 and (mine[0][nan] == 0).all() and (mine[1][nan] == -1).all()


@pytest.mark.parametrize("name", S.NON_FINITE)
def test_non_finite_triangle_lies_where_the_reference_is_defined(shapes, name):
    """A light accepted after a NaN length has no material, and the reference dereferences it
    (AreaLight.cpp:35-39, Shader.cpp:122): such a ray has no reference answer.  The scenes keep clear
    of it (shape_scenes._BELOW): the non-finite triangle is the last one of the last leaf the reference
    visits, that leaf holds nothing of the room and lies below every ray origin, so that only rays
    travelling downward reach it, and no random ray of the GPU half ends on such a light."""
    s = shapes(name)
    boxes, off, cnt, order, ntri = s.bvh()
    bad = s.first + 3
    assert ntri == bad + 1
    leaves, st = [], [0]
    while st:  # the reference's visit order: left first
        i = st.pop()
        if cnt[i] > 0:
            leaves.append(i)
        else:
            st += [int(off[i]) + 1, int(off[i])]
    last = leaves[-1]
    members = order[off[last]:off[last] + cnt[last]]
    print("%s: last leaf %s, box %s" % (name, members, boxes[last]))
    assert members[-1] == bad and (members >= s.first).all()
    lowest_origin = S.BASE_LO[1] - 0.25 * (S.BASE_HI[1] - S.BASE_LO[1])
    assert boxes[last][4] < lowest_origin and S.LIGHT_Y > S.BASE_HI[1] + 0.25 * (S.BASE_HI[1] - S.BASE_LO[1])
    _, _, _, hit, _ = s.rays()
    assert not ((hit[0] == 3) & (hit[1] < 0)).any()  # (the oracle's record of a light without its material)
    assert np.isnan(hit[2]).sum() > 100              # ... while many rays do end on a NaN length


@pytest.mark.parametrize("name", ALL)
def test_scenes_show_something(shapes, name):
    s = shapes(name)
    hit = float((s.hits()[0] > 0).mean())
    bm, rays = s.frame(WHITTED, 1)
    values = len(np.unique(bm))
    print("%s: %.1f %% of the pixels hit, %d distinct pixel values, %d rays" % (name, 100 * hit, values, rays))
    assert hit >= 0.5 and values > 16
    assert not (bm == sentinel(1)[0]).any()


def test_stack_copies_are_hit_and_one_wins(shapes):
    """The coincident copies tie at the same t exactly; the reference's walk settles which one a
    pixel shows (each has its own Kd), the same one on every pixel of the stack."""
    for n in S.STACK_CASES:
        s = shapes("stack%d" % n)
        kind, index, _ = s.hits()
        on = (kind == 3) & (index >= s.first)
        winners = np.unique(index[on])
        print("stack(%d): %d pixels on the stack, winner: copy %s" % (n, int(on.sum()), winners - s.first))
        assert on.mean() > 0.1 and len(winners) == 1


# ---- CPU 2: build parity ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base"] + ALL)
def test_build_equals_the_reference_build(shapes, name):
    """test_parallel_bvh_build_equals_reference_build's comparison: node by node in depth-first
    order (the two arrays place their nodes differently) the box as its bytes, so that NaN and inf
    compare, the triangle count and a leaf's offset; then the primitive order."""
    import mobileraytracer_amd as m
    s = shapes(name)
    boxes, off, cnt, order = m.triangle_bvh(s.cfg())
    oboxes, ooff, ocnt, oorder, _ = s.bvh()
    mine, ref = _bvh_walk(boxes, off, cnt), _bvh_walk(oboxes, ooff, ocnt)
    assert len(mine) == len(ref) == len(ocnt)
    assert mine == ref
    assert np.array_equal(order, oorder)


# ---- CPU 3: the walk tree -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", QUANTIZED)
def test_walk_tree_holds_the_reference_leaves(shapes, name):
    check_walk_tree_holds_reference_leaves(shapes(name).cfg())


@pytest.mark.parametrize("name", S.NON_FINITE)
def test_non_finite_scenes_have_no_quantized_tree(shapes, name):
    import mobileraytracer_amd as m
    cfg = shapes(name).cfg()
    assert m.walk_stack(cfg)["quantized"] is False
    with pytest.raises(RuntimeError, match="not quantizable"):
        m.walk_tree(cfg)


# ---- CPU 4: the stack need ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base"] + ALL)
def test_stack_need_covers_the_reference_tree(shapes, name):
    import mobileraytracer_amd as m
    s = shapes(name)
    w = m.walk_stack(s.cfg())
    _, off, cnt, _, _ = s.bvh()
    depth = depth_of(off, cnt)
    print(name, w)
    assert w["refDepth"] == depth
    assert w["need"] >= depth + 2 and w["need"] >= w["walkDepth"] + 2 and w["need"] >= 3 * w["wideDepth"] + 2
    assert w["spillDepth"] >= w["need"] - 8  # kLdsStackMin
    assert w["quantized"] == (name not in S.NON_FINITE)
    if name.startswith("stack"):
        assert w["need"] == S.STACK_CASES[int(name[5:])][1]


def test_stack_family_straddles_the_packet_limit():
    needs = sorted(need for _, need in S.STACK_CASES.values())
    below = [x for x in needs if x <= PACKET_STACK]
    above = [x for x in needs if x > PACKET_STACK]
    assert len(below) >= 2 and len(above) >= 2
    assert PACKET_STACK in below  # the limit itself is served
    # within one level of the wide tree (kWalkWidth - 1 = 3 entries) on either side, two levels for the second
    assert below[-2] >= PACKET_STACK - 3 and above[0] <= PACKET_STACK + 3 and above[1] <= PACKET_STACK + 6
    assert S.STACK_CASES[S.STACK_DEEP][1] > 400


# ---- CPU 5: the spill stacks' guard -------------------------------------------------------------------
# the most walk threads a device of this family holds: 256 CUs x 4 SIMDs x 8 waves x 64 lanes
MAX_WALK_THREADS = 256 * 2048


def test_spill_stacks_fit_the_offsets_and_are_refused_beyond():
    """A thread's spill area starts at the 32-bit word offset thread * gdepth * 2 (makeRefStack; the
    8-byte entries of makeKeyStack at thread * gdepth).  For the largest launch the deepest tree the
    reference accepts (depth 511: a need of at most 3 * 511 + 2 were the wide tree as deep) stays
    below 2^31 words; a need that does not is refused at load, and so is one whose two areas do not
    fit the memory left beside the queues."""
    import mobileraytracer_amd as m
    deep_need = S.STACK_CASES[S.STACK_DEEP][1]
    for need in (14, deep_need, 513, 3 * 511 + 2):
        gdepth = max(1, need - 8)
        assert MAX_WALK_THREADS * gdepth * 2 < 2 ** 31
        assert m.plan_spill(MAX_WALK_THREADS, need) == 2 * MAX_WALK_THREADS * gdepth * 8
    # the deep case: 3.7 GB on the largest device, far below the half of the device memory that the
    # queue planner leaves free (its budget is the other half)
    assert m.plan_spill(MAX_WALK_THREADS, deep_need) < 4 << 30
    last_ok = (2 ** 31 - 1) // (2 * MAX_WALK_THREADS) + 8
    assert m.plan_spill(MAX_WALK_THREADS, last_ok) > 0
    with pytest.raises(RuntimeError, match="too deep for the walks' spill stacks"):
        m.plan_spill(MAX_WALK_THREADS, last_ok + 1)
    need_bytes = m.plan_spill(MAX_WALK_THREADS, deep_need)
    assert m.plan_spill(MAX_WALK_THREADS, deep_need, need_bytes) == need_bytes
    with pytest.raises(RuntimeError, match="too deep for the device memory"):
        m.plan_spill(MAX_WALK_THREADS, deep_need, need_bytes - 1)
    for bad in ((0, 14), (-1, 14), (2 ** 31 + 1, 14), (64, 2 ** 24 + 9)):
        with pytest.raises(RuntimeError):
            m.plan_spill(*bad)


# ======================================================================================================
# GPU
# ======================================================================================================
def render(r):
    bm = sentinel(SIZE * SIZE)
    r.render_frame(bm)
    return bm


def frame_and_counts(r):
    bm = render(r)
    st = r.frame_stats()
    return bm, (st["rays"], st["shadowRays"], tuple(st["levelRays"]), tuple(st["levelShadowRays"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_primary_hits_equal_the_oracle(shapes, name):
    import mobileraytracer_amd as m
    s = shapes(name)
    with m.Renderer(s.cfg()) as r:
        got = r.primary_hits()
    assert same_hits(got, s.hits())


@pytest.mark.gpu
@pytest.mark.parametrize("shader,spp", [(WHITTED, 1), (PATH_TRACER, 2)])
@pytest.mark.parametrize("name", ALL)
def test_frames_equal_the_oracle(shapes, name, shader, spp):
    import mobileraytracer_amd as m
    s = shapes(name)
    ref, ref_rays = s.frame(shader, spp)
    with m.Renderer(s.cfg(shader, spp)) as r:
        bm = render(r)
        rays = r.get_total_casted_rays()
    assert np.array_equal(bm, ref), int((bm != ref).sum())
    assert rays == ref_rays


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_random_rays_equal_the_oracle(shapes, name):
    import mobileraytracer_amd as m
    s = shapes(name)
    o, d, dist, hit, occ = s.rays()
    rate, occluded = float((hit[0] > 0).mean()), float(occ.mean())
    print("%s: closest-hit rate %.3f, occluded %.3f" % (name, rate, occluded))
    assert rate > 0.2 and 0.02 < occluded < 0.98
    with m.Renderer(s.cfg()) as r:
        got = r.trace_rays(o, d)
        got_occ = r.trace_rays(o, d, dist=dist, any_hit=True)[0]
    assert same_hits(got, hit)
    assert np.array_equal(got_occ, occ)


@pytest.mark.gpu
@pytest.mark.parametrize("name", STACKS)
def test_packet_walk_is_on_exactly_up_to_its_stack(shapes, name):
    """Tuning key 16 is on at load exactly when the need (key 40, the host's mrt_walk_stack) is at
    most 128; above, turning it on is refused; on either side the frame with the per-lane walk is
    the default's, fused and in separate launches."""
    import mobileraytracer_amd as m
    s = shapes(name)
    with m.Renderer(s.cfg()) as r:
        need = r.get_tuning(40)
        assert need == m.walk_stack(s.cfg())["need"] == S.STACK_CASES[int(name[5:])][1]
        with pytest.raises(RuntimeError):
            r.set_tuning(40, need)  # read-only
        assert r.get_tuning(16) == (1 if need <= PACKET_STACK else 0)
        first = frame_and_counts(r)
        hits = r.primary_hits()
        if need > PACKET_STACK:
            with pytest.raises(RuntimeError, match="deeper stack"):
                r.set_tuning(16, 1)
            assert r.get_tuning(16) == 0
        else:
            r.set_tuning(16, 1)
        outs = []
        for packet, fuse in ((0, -1), (0, 0), (r.get_tuning(16), 0), (r.get_tuning(16), 1)):
            r.set_tuning(16, packet)
            r.set_tuning(17, fuse)
            outs.append((frame_and_counts(r), r.primary_hits()))
    assert np.array_equal(first[0], s.frame(WHITTED, 1)[0])
    for (bm, counts), h in outs:
        assert np.array_equal(bm, first[0]) and counts == first[1]
        assert same_hits(h, hits)


# test_walk_and_cull_settings_give_identical_results's settings (tests/test_cast_rays_gpu.py), then the
# certified cull mode, level 1 in separate launches (with the packet walk generating the camera rays
# or k_raygen) and the per-lane walk for the camera rays
SETTINGS = [((1, 0),), ((2, 0),), ((2, 3),), ((28, 1),), ((1, 0), (28, 1)),
            ((2, 2),), ((17, 0),), ((17, 0), (33, 0)), ((16, 0),), ((16, 0), (2, 0))]


@pytest.mark.gpu
@pytest.mark.parametrize("shader,spp", [(WHITTED, 1), (PATH_TRACER, 2)])
@pytest.mark.parametrize("name", [DEEP] + list(S.SCENES))
def test_walk_and_cull_settings_change_nothing(shapes, name, shader, spp):
    """Frames, ray counts, primary hits and the random rays' results under every walk and cull
    setting equal the default's (and with it the oracle's)."""
    import mobileraytracer_amd as m
    s = shapes(name)
    o, d, dist, hit, occ = s.rays()
    ref, _ = s.frame(shader, spp)
    with m.Renderer(s.cfg(shader, spp)) as r:
        packet = r.get_tuning(16)
        default = frame_and_counts(r)
        assert np.array_equal(default[0], ref)
        for setting in SETTINGS:
            for key, value in ((1, 1), (2, 3), (28, 0), (17, -1), (33, 2), (16, packet)) + setting:
                r.set_tuning(key, value)
            bm, counts = frame_and_counts(r)
            assert np.array_equal(bm, default[0]), setting
            assert counts == default[1], setting
            if shader == WHITTED:
                assert same_hits(r.primary_hits(), s.hits()), setting
                assert same_hits(r.trace_rays(o, d), hit), setting
                assert np.array_equal(r.trace_rays(o, d, dist=dist, any_hit=True)[0], occ), setting


def views():
    """CAMS as Renderer.render_views takes them (what the loader makes of the .cam text at a square
    frame: position X negated, hFov = f.u * 1)."""
    return [(0, (-p[0], p[1], p[2]), l, (0.0, 1.0, 0.0), f[0], f[1]) for p, l, f in CAMS]


@pytest.mark.gpu
@pytest.mark.parametrize("shader,spp", [(WHITTED, 1), (PATH_TRACER, 2)])
def test_deep_stack_batch_of_views_equals_the_single_frames(shapes, shader, spp):
    import mobileraytracer_amd as m
    s = shapes(DEEP)
    with m.Renderer(s.cfg(shader, spp)) as r:
        own = render(r)
        singles, rays = sentinel(2, SIZE * SIZE), []
        for v, cam in enumerate(views()):
            before = r.get_total_casted_rays()
            r.set_camera(*cam)
            r.render_frame(singles[v])
            rays.append(r.get_total_casted_rays() - before)
    assert np.array_equal(singles[0], own) and np.array_equal(own, s.frame(shader, spp)[0])
    assert not np.array_equal(singles[0], singles[1])
    with m.Renderer(s.cfg(shader, spp)) as r:
        bms = sentinel(2, SIZE * SIZE)
        r.render_views(views(), bms)
        assert np.array_equal(bms, singles)
        assert r.get_total_casted_rays() == sum(rays)


@pytest.mark.gpu
@pytest.mark.parametrize("shader,spp", [(WHITTED, 1), (PATH_TRACER, 2)])
def test_deep_stack_two_shards_assemble_to_the_single_frame(shapes, shader, spp):
    """Two rank shards, each its packed half into device memory, unpacked by rank 0 (the assembly of
    test_two_shards_replan_each_for_itself)."""
    import torch
    import mobileraytracer_amd as m
    s = shapes(DEEP)
    ref, ref_rays = s.frame(shader, spp)
    rs = [m.Renderer(dataclasses.replace(s.cfg(shader, spp), rankIndex=k, rankCount=2)) for k in range(2)]
    try:
        slots_max = rs[0].scene_info()["pixelSlotsMax"]
        gathered = torch.zeros((2, slots_max), dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for k, r in enumerate(rs):
            r.render_frame_device(0, gathered[k].data_ptr(), stream)
        torch.cuda.synchronize()
        out = torch.full((SIZE * SIZE,), int(sentinel(1)[0]), dtype=torch.int32, device="cuda")
        rs[0].unpack_gathered(gathered.data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref)
        assert sum(r.get_total_casted_rays() for r in rs) == ref_rays
    finally:
        for r in rs:
            r.close()
