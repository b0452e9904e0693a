"""The wavefront queue planner (mrt_plan_queues, host only): the first allocation, the plan after an
overflowed pass, the worst-case plan, the byte budget and the int range."""
import pytest

import mobileraytracer_amd as m

SEGS = 8
RAY_BYTES = 16 + 16 + 4 + 16 + 16 + 16   # rO rD tree hit vtx res
SHADOW_BYTES = 3 * 16                    # sO sD sC
LIMIT = 1 << 30


@pytest.fixture(scope="module", autouse=True)
def _lib(native_lib_path):
    return native_lib_path


def first_formula(n1, spl, levels):
    """allocQueues' sizes before the planner: level 1 dense, deeper levels 2 x level 1 x 1.25 over 8
    segments plus 3072 slots, shadow queues the same with 1024 slots per light sample."""
    seg, sh = [], []
    for lv in range(1, levels + 1):
        if lv == 1:
            seg.append((n1 + 7) // 8)
            sh.append((n1 * spl * 5 // 4 + 7) // 8 + spl * 1024)
        else:
            seg.append((2 * n1 * 5 // 4 + 7) // 8 + 3072)
            sh.append((2 * n1 * spl * 5 // 4 + 7) // 8 + spl * 1024)
    return seg, sh


def plan_bytes(p, textured=False):
    ray = RAY_BYTES + (32 if textured else 0)
    return SEGS * sum(s * ray + h * SHADOW_BYTES for s, h in zip(p["segCap"], p["shadowSegCap"]))


@pytest.mark.parametrize("slots,spp,spl,branching", [
    (1920 * 1080, 4, 1, 3),   # C4: 1080p PathTracer, 4 spp: 8.3 M paths in one chunk
    (64 * 64, 1, 1, 2),       # the small frames of the suite
    (64 * 64, 2, 3, 3),
])
def test_first_allocation_is_the_fixed_growth_formula(slots, spp, spl, branching):
    p = m.plan_queues(levels=7, branching=branching, pixel_slots=slots, samples_pixel=spp, samples_light=spl)
    assert p["chunkSlots"] == slots and not p["worstCase"]
    seg, sh = first_formula(slots * spp, spl, 7)
    assert p["segCap"] == seg and p["shadowSegCap"] == sh
    assert p["bytes"] == plan_bytes(p)


def test_first_allocation_keeps_the_path_budget():
    p = m.plan_queues(levels=7, branching=3, pixel_slots=1 << 20, samples_pixel=4, path_budget=1 << 16)
    assert p["chunkSlots"] == (1 << 16) // 4
    seg, sh = first_formula(1 << 16, 1, 7)
    assert p["segCap"] == seg and p["shadowSegCap"] == sh


# a synthetic overflowed pass: 16384 paths in one chunk, 7 levels, level 5 the first to overflow.
# Segment demands are deliberately uneven: level 4's largest segment holds twice its mean.
N1 = 16384
DEMAND = {
    "mask": (1 << 5) | (1 << 6), "chunkSlots": N1, "paths": N1,
    #        L1    L2    L3    L4     L5     L6     L7
    "seg": [2048, 3000, 5000, 9000, 15000, 9000, 7000],        # L5 asked for 15000 > its 8192
    "shadowSeg": [1500, 2500, 4000, 7000, 3000, 2000, 0],
}


def first16k():
    return m.plan_queues(levels=7, branching=2, pixel_slots=N1)


def test_demand_plan_sizes_exact_levels_from_the_largest_segment():
    prev = first16k()
    assert prev["segCap"][4] == 8192 and DEMAND["seg"][4] > prev["segCap"][4]
    p = m.plan_queues(levels=7, branching=2, pixel_slots=N1, demand=DEMAND, previous=prev)
    assert p["chunkSlots"] == N1
    # exact ray levels 2..5: ceil(1.25 x the largest segment) + slack, whatever the mean was
    for lv in (2, 3, 4, 5):
        assert p["segCap"][lv - 1] == max(prev["segCap"][lv - 1], -(-DEMAND["seg"][lv - 1] * 5 // 4) + 3072)
    assert p["segCap"][3] == 9000 * 5 // 4 + 3072  # not 1.25 x a mean of 4500
    assert p["segCap"][0] == N1 // 8               # level 1 stays dense
    # exact shadow levels 1..4 (level 5's rays were dropped, so its shadow count is a lower bound)
    for lv in (1, 2, 3, 4):
        assert p["shadowSegCap"][lv - 1] == max(prev["shadowSegCap"][lv - 1],
                                                -(-DEMAND["shadowSeg"][lv - 1] * 5 // 4) + 1024)


def test_demand_plan_extrapolates_deeper_levels_and_respects_lower_bounds():
    prev = first16k()
    p = m.plan_queues(levels=7, branching=2, pixel_slots=N1, demand=DEMAND, previous=prev)
    ratio = 15000 / 9000  # observed level 4 -> 5, inside [1, 2]
    e6 = 15000 * ratio
    e7 = e6 * ratio
    assert abs(p["segCap"][5] - (e6 * 1.25 + 3072)) <= 4
    assert abs(p["segCap"][6] - (e7 * 1.25 + 3072)) <= 8
    # never below the lower bound the pass reported
    for lv in (6, 7):
        assert p["segCap"][lv - 1] >= DEMAND["seg"][lv - 1] * 5 // 4 + 3072
    # a lower bound above the extrapolation wins
    d = dict(DEMAND, seg=DEMAND["seg"][:6] + [90000])
    p2 = m.plan_queues(levels=7, branching=2, pixel_slots=N1, demand=d, previous=prev)
    assert p2["segCap"][6] == 90000 * 5 // 4 + 3072
    # the ratio is clamped to the shader's branching bound ...
    d = dict(DEMAND, seg=[2048, 100, 200, 300, 15000, 0, 0])
    p3 = m.plan_queues(levels=7, branching=2, pixel_slots=N1, demand=d, previous=prev)
    assert p3["segCap"][5] == 30000 * 5 // 4 + 3072 and p3["segCap"][6] == 60000 * 5 // 4 + 3072
    # ... and to 1 from below: a shrinking tree is not trusted to keep shrinking
    d = dict(DEMAND, seg=[2048, 9000, 9000, 20000, 10000, 0, 0], mask=1 << 5)
    p4 = m.plan_queues(levels=7, branching=2, pixel_slots=N1, demand=d, previous=prev)
    assert p4["segCap"][5] == p4["segCap"][4] == 10000 * 5 // 4 + 3072


def test_demand_plan_fits_the_budget_and_keeps_capacity_per_path():
    prev = first16k()
    full = m.plan_queues(levels=7, branching=2, pixel_slots=N1, demand=DEMAND, previous=prev)
    assert full["bytes"] == plan_bytes(full)
    budget = full["bytes"] // 2
    half = m.plan_queues(levels=7, branching=2, pixel_slots=N1, demand=DEMAND, previous=prev, byte_budget=budget)
    assert half["bytes"] == plan_bytes(half) <= budget
    assert half["chunkSlots"] < full["chunkSlots"]
    # the largest chunk that fits: one more slot would not
    quarter = m.plan_queues(levels=7, branching=2, pixel_slots=N1, demand=DEMAND, previous=prev,
                            byte_budget=budget // 2)
    assert quarter["bytes"] <= budget // 2 and quarter["chunkSlots"] < half["chunkSlots"]
    # capacity per path beyond the fixed slack is the same for every chunk, up to rounding: the
    # scaled demand and its 1.25 are each rounded up once (-1 .. +4 slots); an extrapolated level
    # multiplies k times by a ratio of two scaled, rounded-up demands, each within 1 of exact, so
    # the ratio is within 2 / (the smaller demand) relatively, per step; the shadow rays per ray
    # likewise, from the smallest exact shadow demand (1500 x scale)
    for small in (half, quarter):
        scale = small["chunkSlots"] / full["chunkSlots"]
        for lv in range(2, 8):
            want = (full["segCap"][lv - 1] - 3072) * scale
            rel = max(0, lv - 5) * 2 / (9000 * scale)
            assert want * (1 - rel) - 1 - 3 * max(0, lv - 5) <= small["segCap"][lv - 1] - 3072 \
                <= want * (1 + rel) + 4 + 3 * max(0, lv - 5), lv
        for lv in range(1, 8):
            want = (full["shadowSegCap"][lv - 1] - 1024) * scale
            rel = (max(0, lv - 5) * 2 / (9000 * scale) + 2 / (1500 * scale)) if lv > 4 else 0
            assert want * (1 - rel) - 1 - 6 * max(0, lv - 4) <= small["shadowSegCap"][lv - 1] - 1024 \
                <= want * (1 + rel) + 4 + 6 * max(0, lv - 4), lv


def test_capacities_never_shrink_across_plans():
    prev = first16k()
    p1 = m.plan_queues(levels=7, branching=2, pixel_slots=N1, demand=DEMAND, previous=prev)
    # a later pass (another camera) asks for much less on the early levels and overflows level 7
    d2 = {"mask": 1 << 7, "chunkSlots": N1, "paths": N1,
          "seg": [2048, 100, 200, 300, 400, 500, p1["segCap"][6] + 1000],
          "shadowSeg": [10, 10, 10, 10, 10, 10, 0]}
    p2 = m.plan_queues(levels=7, branching=2, pixel_slots=N1, demand=d2, previous=p1)
    for lv in range(1, 8):
        assert p2["segCap"][lv - 1] >= p1["segCap"][lv - 1] >= prev["segCap"][lv - 1]
        assert p2["shadowSegCap"][lv - 1] >= p1["shadowSegCap"][lv - 1] >= prev["shadowSegCap"][lv - 1]
    assert p2["segCap"][6] == -(-(p1["segCap"][6] + 1000) * 5 // 4) + 3072
    # ... and per path when the chunk shrinks with the budget
    p3 = m.plan_queues(levels=7, branching=2, pixel_slots=N1, demand=d2, previous=p1, byte_budget=p2["bytes"] // 3)
    assert p3["chunkSlots"] < N1
    for lv in range(2, 8):
        assert p3["segCap"][lv - 1] * N1 >= p1["segCap"][lv - 1] * p3["chunkSlots"]


def test_progressive_demand_scales_by_the_paths_the_pass_ran():
    # spp 4, progressive: the queues are allocated for 4 samples per slot, a pass runs 1
    prev = m.plan_queues(levels=3, branching=2, pixel_slots=4096, samples_pixel=4)
    d = {"mask": 1 << 2, "chunkSlots": 4096, "paths": 4096, "seg": [512, 30000, 0], "shadowSeg": [400, 0, 0]}
    p = m.plan_queues(levels=3, branching=2, pixel_slots=4096, samples_pixel=4, demand=d, previous=prev)
    assert p["segCap"][1] == 30000 * 5 // 4 + 3072   # not 4 x that
    assert p["segCap"][0] == 4096 * 4 // 8


def test_worst_case_plan_holds_the_whole_ray_tree():
    n1 = 8 * 256 * 5  # whole 256-vertex blocks per segment: the bound is exact
    p = m.plan_queues(levels=7, branching=3, pixel_slots=n1, samples_light=2, worst_case=True)
    assert p["worstCase"] and p["chunkSlots"] == n1
    for lv in range(1, 8):
        assert SEGS * p["segCap"][lv - 1] == n1 * 3 ** (lv - 1)
        assert SEGS * p["shadowSegCap"][lv - 1] == 2 * n1 * 3 ** (lv - 1)
    assert p["bytes"] == plan_bytes(p)
    # an odd size: at least the tree, at most one 256-block of parents per segment and level more
    p = m.plan_queues(levels=7, branching=3, pixel_slots=1000, samples_pixel=3, samples_light=2, worst_case=True)
    assert p["chunkSlots"] == 1000
    for lv in range(2, 8):
        tree = 3000 * 3 ** (lv - 1)
        assert tree <= SEGS * p["segCap"][lv - 1] <= tree + SEGS * 256 * 3 ** (lv - 1)
        assert SEGS * p["shadowSegCap"][lv - 1] >= 2 * tree


def test_worst_case_plan_fits_the_budget_or_reports_the_one_pixel_error():
    n1 = 128 * 128
    free = m.plan_queues(levels=7, branching=3, pixel_slots=n1, samples_light=2, worst_case=True)
    budget = 64 << 20
    assert free["bytes"] > budget
    p = m.plan_queues(levels=7, branching=3, pixel_slots=n1, samples_light=2, worst_case=True, byte_budget=budget)
    assert p["worstCase"] and p["bytes"] == plan_bytes(p) <= budget and 1 <= p["chunkSlots"] < n1
    more = m.plan_queues(levels=7, branching=3, pixel_slots=p["chunkSlots"] + 1, samples_light=2, worst_case=True)
    assert more["bytes"] > budget  # the largest chunk that fits
    # one slot's tree: (3^7 - 1) / 2 = 1093 rays and 2 x 1093 shadow rays
    one = m.plan_queues(levels=7, branching=3, pixel_slots=1, samples_light=2, worst_case=True)
    assert one["bytes"] >= 1093 * RAY_BYTES + 2186 * SHADOW_BYTES
    with pytest.raises(RuntimeError, match="one pixel's worst-case ray tree does not fit"):
        m.plan_queues(levels=7, branching=3, pixel_slots=n1, samples_light=2, worst_case=True,
                      byte_budget=one["bytes"] - 1)
    assert m.plan_queues(levels=7, branching=3, pixel_slots=n1, samples_light=2, worst_case=True,
                         byte_budget=one["bytes"])["chunkSlots"] == 1


def test_path_budget_is_bounded():
    with pytest.raises(RuntimeError):
        m.plan_queues(levels=7, branching=2, pixel_slots=64, path_budget=1 << 40)


def test_textured_slots_are_larger():
    a = m.plan_queues(levels=7, branching=2, pixel_slots=4096)
    b = m.plan_queues(levels=7, branching=2, pixel_slots=4096, textured=True)
    assert a["segCap"] == b["segCap"] and b["bytes"] == plan_bytes(b, textured=True) > a["bytes"]


def test_everything_stays_below_2_30_at_4k_8spp():
    slots, spp = 3840 * 2160, 8
    first = m.plan_queues(levels=7, branching=3, pixel_slots=slots, samples_pixel=spp, samples_light=4)
    worst = m.plan_queues(levels=7, branching=3, pixel_slots=slots, samples_pixel=spp, samples_light=4,
                          worst_case=True)
    # a pass whose level 3 asked for 40 x level 1 in one segment
    n1 = first["chunkSlots"] * spp
    d = {"mask": 1 << 3, "chunkSlots": first["chunkSlots"], "paths": n1,
         "seg": [n1 // 8, n1 // 4, 5 * n1, 0, 0, 0, 0], "shadowSeg": [n1 // 2, n1, 0, 0, 0, 0, 0]}
    after = m.plan_queues(levels=7, branching=3, pixel_slots=slots, samples_pixel=spp, samples_light=4,
                          demand=d, previous=first)
    for p in (first, worst, after):
        assert p["chunkSlots"] >= 1
        for lv in range(7):
            assert 0 < SEGS * p["segCap"][lv] < LIMIT and 0 <= SEGS * p["shadowSegCap"][lv] < LIMIT
    assert first["chunkSlots"] == (1 << 24) // spp        # the path budget alone
    assert worst["chunkSlots"] < first["chunkSlots"]      # 3^6 x level 1 x 4 shadow rays: a smaller chunk
    assert after["chunkSlots"] < first["chunkSlots"]
    # the demand the plan was sized for is below the limit too: 1.25 x it is the capacity
    scale = after["chunkSlots"] / first["chunkSlots"]
    assert 5 * n1 * scale < LIMIT


def test_malformed_requests_are_refused():
    with pytest.raises(RuntimeError):
        m.plan_queues(levels=0, branching=2, pixel_slots=64)
    with pytest.raises(RuntimeError):
        m.plan_queues(levels=7, branching=2, pixel_slots=64,
                      demand={"mask": 0, "chunkSlots": 64, "paths": 64, "seg": [8] * 7, "shadowSeg": [0] * 7})
