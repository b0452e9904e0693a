"""Overlap queries (mrt_overlap_boxes_device): the surfaces touching each box, in (kind, input index) order,
and their number.  Every comparison is exact on ints against lists built on the host: mrt_box_overlap on
every candidate of the scene accessors, the documented order applied in NumPy (overlap_cases.Lists).  Each
case runs with three field sets - all fields, all but `count`, `any` only (the form that stops at the first
acceptance) - and under BVH and Naive unless it says otherwise.  `tests` is diagnostic and compared nowhere,
only bounded where the cull is the subject.

Frames are 16 x 16; outputs given to the C entry point start filled with a sentinel."""
import dataclasses

import numpy as np
import pytest

import neighbour_cases as NB
import overlap_cases as C
import shape_scenes as S
from test_cast_rays_gpu import SENTINEL, bits, dev

pytestmark = pytest.mark.gpu

f32 = np.float32
NAIVE, GRID, BVH = 1, 2, 3
ALL = tuple(C.WIDTHS)
NO_COUNT = tuple(f for f in ALL if f != "count")
ANY = ("any", "tests")  # (`tests` does not change the form)
FORMS = (ALL, NO_COUNT, ANY)


def query(r, boxes, k, fields=None):
    b = dev(np.ascontiguousarray(boxes, f32))
    got = r.overlap_boxes(b[:, :3], b[:, 3:], k, fields=fields)
    return {f: x.cpu().numpy() for f, x in got.items()}


def every_form(cfg, jobs, accelerators=(BVH, NAIVE)):
    """jobs: (what, boxes, k, want).  Each job under each accelerator with each field set: every answer equals
    the host's, so the accelerators and the forms equal each other bit for bit.  Returns the answers by
    (accelerator, what, field set)."""
    import mobileraytracer_amd as m
    out = {}
    for acc in accelerators:
        with m.Renderer(dataclasses.replace(cfg, accelerator=acc)) as r:
            for what, boxes, k, want in jobs:
                for fields in FORMS:
                    got = query(r, boxes, k, fields=fields)
                    assert set(got) == set(fields)
                    C.assert_same(got, want, "%s, K = %d, accelerator %d, fields %s" % (what, k, acc, fields))
                    if "count" in got:
                        assert np.array_equal(got["any"], (got["count"] > 0).astype(np.int32))
                    out[acc, what, fields] = got
    return out


# ---- 1. the device's functions are the host's ---------------------------------------------------------
@pytest.mark.parametrize("kind", [C.PLANE, C.SPHERE, C.TRIANGLE, C.LIGHT])
def test_kat_box_overlap_is_box_overlap(kind):
    import mobileraytracer_amd as m
    n = 1 << 16
    if kind in (C.TRIANGLE, C.LIGHT):
        parts = [C.triangle_pairs(n // 4, 200 + kind + int(off), off) for off in C.OFFSETS]
        prims, boxes = np.concatenate([p for p, _ in parts]), np.concatenate([b for _, b in parts])
    else:
        prims, boxes = (C.plane_pairs if kind == C.PLANE else C.sphere_pairs)(n, 200 + kind)
    boxes[::97, 3] = np.nan  # (and some invalid boxes)
    boxes[5::101, 1] = np.inf
    host = m.box_overlap(kind, prims, boxes)
    assert 0.05 < host.mean() < 0.5 and (host[::97] == 0).all()
    assert np.array_equal(m.kat_box_overlap(kind, prims, boxes), host)


# ---- 2. a soup: every field, K = 1, 4, 16, truncation ---------------------------------------------------
def soup_case(path, offset, size):
    import mobileraytracer_amd as m
    cfg = NB.obj_cfg(NB.soup(path, "soup", offset, size))
    geom = m.scene_triangles(cfg)[0]
    assert len(geom) == 300
    boxes = C.scene_boxes(geom, 600, 33, 1.0 + 6 * size)
    lists = C.Lists(cfg)
    ok = lists.accepted(boxes)
    case = {"cfg": cfg, "geom": geom, "boxes": boxes, "lists": lists, "ok": ok,
            "want": {k: lists.expected(boxes, k, ok=ok) for k in (1, 4, 16)}}
    for x in (boxes, ok):
        x.setflags(write=False)
    return case


@pytest.fixture(scope="module")
def soup0(tmp_path_factory):
    """The soup at the origin, 600 boxes (points of the surface, corners, cubes, slabs, the whole scene box and
    boxes touching its faces), the host's verdict on all 302 candidates and the lists for K = 1, 4 and 16."""
    return soup_case(str(tmp_path_factory.mktemp("overlap_soup")), 0.0, 0.2)


def check_soup(case, what):
    want = case["want"]
    count = want[16]["count"]
    assert count[-4] >= 300 and (count[:200] >= 1).mean() > 0.95  # (the whole scene box; points of the surface)
    assert (count == 0).sum() >= 20 and (count > 16).sum() >= 20 and ((count > 0) & (count < 16)).sum() >= 100
    for k in (1, 4):  # (on the host: a shorter list is the longer one cut)
        C.assert_same(C.cut(want[16], k), want[k], "the host's own K = %d" % k)
    got = every_form(case["cfg"], [("%s, %d" % (what, k), case["boxes"], k, want[k]) for k in (1, 4, 16)])
    for acc in (BVH, NAIVE):
        for fields in (ALL, NO_COUNT):
            long = got[acc, what + ", 16", fields]
            for k in (1, 4):
                C.assert_same(got[acc, "%s, %d" % (what, k), fields], C.cut(long, k), "%s: K = %d against the K = 16 list" % (what, k))
    assert (got[NAIVE, what + ", 16", ALL]["tests"][np.isfinite(case["boxes"]).all(1)] == 302).all()


def test_soup_at_the_origin(soup0):
    check_soup(soup0, "soup at 0")


def test_soup_at_1024(tmp_path):
    check_soup(soup_case(str(tmp_path), 1024.0, 0.01), "soup at 1024")


# ---- 3. counts of 0, 1, K - 1, K, K + 1 and every candidate ----------------------------------------------
def test_counts_around_k_on_two_sheets(tmp_path):
    """Two 16 x 16 sheets of unit quads (z = 0 and z = 2).  Thin boxes at the lower sheet, placed
    against the cells' diagonals, are chosen for counts of 0, 1, K - 1, K, K + 1 and every candidate
    (K = 4), asserted on the host first."""
    import mobileraytracer_amd as m
    K = 4
    cfg = NB.obj_cfg(NB.write_mesh(str(tmp_path), "sheets", quads=NB.sheet_quads(16, 0) + NB.sheet_quads(16, 2), light=NB.FAR_LIGHT))
    geom = m.scene_triangles(cfg)[0]
    assert len(geom) == 1024
    lists = C.Lists(cfg)
    lo = NB.corners_of(geom).min(0).astype(np.float64)
    rng = np.random.default_rng(35)
    rows = []
    for i in range(96):
        x, y = lo[:2] + rng.integers(1, 12, 2)
        c = i % 6
        if c == 0:    # between the sheets
            rows.append((x + 0.1, y + 0.1, lo[2] + 0.5, x + 3.9, y + 3.9, lo[2] + 1.5))
        elif c == 1:  # inside a cell's lower-right triangle (the loaded quads are cut along y = x from the cell's corner)
            rows.append((x + 0.6, y + 0.1, lo[2] - 0.1, x + 0.9, y + 0.3, lo[2] + 0.1))
        elif c == 2:  # both triangles of one cell and the upper-left one of the next: 3
            rows.append((x + 0.6, y + 0.6, lo[2] - 0.1, x + 1.4, y + 0.9, lo[2] + 0.1))
        elif c == 3:  # both triangles of two cells: 4
            rows.append((x + 0.3, y + 0.45, lo[2] - 0.1, x + 1.7, y + 0.55, lo[2] + 0.1))
        elif c == 4:  # two, two and one: 5
            rows.append((x + 0.6, y + 0.6, lo[2] - 0.1, x + 2.4, y + 0.9, lo[2] + 0.1))
        else:         # everything
            rows.append((lo[0] - 1, lo[1] - 1, lo[2] - 1, lo[0] + 17, lo[1] + 17, 65))
    boxes = np.array(rows, f32)
    ok = lists.accepted(boxes)
    want = lists.expected(boxes, K, ok=ok)
    classes = (0, 1, K - 1, K, K + 1, len(lists.kind))
    for c, cls in enumerate(classes):  # (on the host, before the GPU is asked)
        assert (want["count"][c::6] == cls).all(), (cls, want["count"][c::6])
    held = np.arange(K)[None, :] < want["count"][:, None]
    assert (want["kind"][~held] == 0).all() and (want["index"][~held] == -1).all()
    full = want["count"] > K  # truncation: the K smallest input indices
    first = np.argsort(~ok[full], axis=1, kind="stable")[:, :K]
    assert np.array_equal(want["index"][full], lists.index[first]) and (np.diff(want["index"][full], axis=1) > 0).all()
    every_form(cfg, [("sheets", boxes, K, want)])


# ---- 4. the cull -----------------------------------------------------------------------------------------
def test_the_walk_tests_only_leaves_that_overlap_the_box(tmp_path):
    """The 46 x 46 sheet: 1,024 small boxes at the sheet, 64 above it that touch nothing.  `tests` is at most the
    triangles of the reference leaves whose boxes overlap the query box (closed compares on triangle_bvh's
    boxes) plus the lights; 0 for a box outside the root.  With `any` only the mean is not above the counted
    form's."""
    import mobileraytracer_amd as m
    cfg = NB.obj_cfg(NB.write_mesh(str(tmp_path), "sheet46", quads=NB.sheet_quads(46, 0), light=NB.FAR_LIGHT))
    geom = m.scene_triangles(cfg)[0]
    T = len(geom)
    assert T == 4232
    lo = NB.corners_of(geom).min(0)
    rng = np.random.default_rng(41)
    c = np.concatenate([lo[:2] + rng.integers(0, 46, (1024, 2)) + rng.random((1024, 2)), np.full((1024, 1), lo[2])], 1)
    h = 10.0 ** rng.uniform(-3, 0, (1024, 1)) * 0.5
    at = np.concatenate([c - h, c + h], 1).astype(f32)
    above = at[:64].copy()
    above[:, 2], above[:, 5] = lo[2] + 1, lo[2] + 2
    boxes = np.concatenate([at, above])
    lists = C.Lists(cfg)
    want = lists.expected(boxes, 16)
    assert (want["count"][:1024] >= 1).all() and (want["count"][1024:] == 0).all()
    nodes, _, cnt, _ = m.triangle_bvh(cfg)
    leaf = cnt > 0
    assert cnt[leaf].sum() == T
    b = nodes[leaf]
    apart = ((b[None, :, :3] > boxes[:, None, 3:]) | (b[None, :, 3:] < boxes[:, None, :3])).any(2)
    reach = ((~apart) * cnt[leaf][None, :]).sum(1)
    got = every_form(cfg, [("sheet", boxes, 16, want)])
    F = 2  # the two far lights, met one by one
    assert (got[NAIVE, "sheet", ALL]["tests"] == T + F).all()
    tests = got[BVH, "sheet", ALL]["tests"]
    fast = got[BVH, "sheet", ANY]["tests"]
    print("46 x 46 sheet: mean count %.1f, mean tests per box %.1f (any only: %.1f), mean triangles in overlapping "
          "leaves %.1f (of %d)" % (want["count"][:1024].mean(), tests.mean(), fast.mean(), reach.mean(), T))
    assert (want["count"] <= tests - F).all() and (tests - F <= reach).all()
    assert (tests[1024:] == F).all() and reach[:1024].mean() < T / 8
    assert (fast <= tests).all() and fast.mean() <= tests.mean()


# ---- 5. tree shapes and bad geometry ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack%d" % S.STACK_DEEP, "degenerate", "inf_vertex", "outlier"])
def test_tree_shapes(tmp_path, name):
    import mobileraytracer_amd as m
    files = S.write_scene(str(tmp_path), name)
    cfg = NB.obj_cfg(files[:3])
    if name.startswith("stack"):
        assert m.walk_stack(cfg)["need"] == S.STACK_CASES[S.STACK_DEEP][1]  # far beyond the LDS stack
    geom = m.scene_triangles(cfg)[0]
    fin = geom[np.isfinite(geom).all((1, 2)) & (np.abs(geom) < 1e6).all((1, 2))]
    boxes = C.scene_boxes(fin, 60, 52, 20.0)
    boxes = np.concatenate([boxes, [(-1e30, -1e30, -1e30, 1e30, 1e30, 1e30), (-3e38, -3e38, -3e38, 3e38, 3e38, 3e38),
                                    (-9, -13, -11, 9, 10, 41), (0, 0, 0, 2.0 ** 41, 2.0 ** 41, 2.0 ** 41)]]).astype(f32)
    lists = C.Lists(cfg)
    ok = lists.accepted(boxes)
    want = lists.expected(boxes, 4, ok=ok)
    bad = ~np.isfinite(lists.rec[C.TRIANGLE]).all(1)
    if name == "inf_vertex":
        assert bad.any()
    t0 = lists.first[C.TRIANGLE]
    assert not ok[:, t0:t0 + len(bad)][:, bad].any()  # a non-finite triangle is never accepted ...
    assert (want["count"][-4:-1] >= (~bad).sum() - 1).all() and (want["count"] > 4).sum() >= 8
    got = every_form(cfg, [(name, boxes, 4, want)])
    big = every_form(cfg, [(name + ", 16", boxes, 16, lists.expected(boxes, 16, ok=ok))], accelerators=(BVH,))
    for res in list(got.values()) + list(big.values()):  # ... and never listed
        if "index" in res:
            assert not (np.isin(res["index"], np.nonzero(bad)[0]) & (res["kind"] == C.TRIANGLE)).any()


# ---- 6. other kinds ----------------------------------------------------------------------------------------
def test_planes_spheres_and_lights_and_no_accelerator():
    """Built-in scenes 1 - 3: boxes about points near every kind's surfaces (found with point_distance), and one
    box that holds everything: its list starts with the planes, then the spheres, the triangles, the lights.
    With an accelerator id that builds nothing only the area lights are candidates."""
    import mobileraytracer_amd as m
    import nearest_cases as N
    seen = set()
    for scene in (1, 2, 3):
        cfg = m.Config(width=16, height=16, shader=1, sceneIndex=scene)
        lists = C.Lists(cfg)
        cands = N.Candidates(cfg)
        pts = NB.builtin_points(cands, 126, 60 + scene).astype(np.float64)
        rng = np.random.default_rng(61 + scene)
        h = 10.0 ** rng.uniform(-3, 0.5, (126, 3)) * 0.5
        h[::7] = 0.0
        boxes = np.concatenate([np.concatenate([pts - h, pts + h], 1), [(-1e4, -1e4, -1e4, 1e4, 1e4, 1e4),
                                                                         (-1e4, -1e4, -1e4, -9e3, -9e3, -9e3)]]).astype(f32)
        ok = lists.accepted(boxes)
        want = lists.expected(boxes, 16, ok=ok)
        kinds = {k: int((want["kind"] == k).sum()) for k in (1, 2, 3, 4)}
        print("scene %d: candidates %s, list entries per kind %s" % (scene, cands.count, kinds))
        seen |= {k for k, c in kinds.items() if c >= 4}
        lkind = m.scene_lights(cfg)[0]
        lit = want["kind"] == C.LIGHT
        assert (lkind[want["index"][lit]] == 1).all()  # a point light never appears
        everything = want["kind"][-2][:want["count"][-2]]
        assert (np.diff(everything) >= 0).all()  # kind order in the box that holds all
        every_form(cfg, [("scene %d" % scene, boxes, 16, want), ("scene %d, 4" % scene, boxes, 4, C.cut(want, 4))])
        lights = C.Lists(cfg, lights_only=True)
        want0 = lights.expected(boxes, 4)
        assert set(np.unique(want0["kind"])) <= {0, C.LIGHT} and want0["count"][-2] == (lkind == 1).sum()
        every_form(cfg, [("scene %d, no accelerator" % scene, boxes, 4, want0)], accelerators=(0,))
    assert seen == {1, 2, 3, 4}


# ---- 7. invalid boxes ------------------------------------------------------------------------------------
def test_invalid_boxes_accept_nothing_and_leave_their_neighbours_alone(soup0):
    boxes = soup0["boxes"][200:328].copy()
    want = C.rows_of(soup0["want"][4], slice(200, 328))
    assert (want["count"] > 0).mean() > 0.5
    bad = np.arange(0, 128, 3)
    for i, row in enumerate(bad):
        slot = i % 6
        if i % 3 == 0:
            boxes[row, slot] = np.nan
        elif i % 3 == 1:
            boxes[row, slot] = np.inf if slot >= 3 else -np.inf
        else:  # mn > mx on one axis
            a = slot % 3
            boxes[row, a], boxes[row, 3 + a] = boxes[row, 3 + a] + 1, boxes[row, a]
    want = {f: x.copy() for f, x in want.items()}
    want["any"][bad], want["count"][bad], want["kind"][bad], want["index"][bad] = 0, 0, 0, -1
    host = soup0["lists"].expected(boxes, 4)
    C.assert_same(host, want, "the host's own answer")
    got = every_form(soup0["cfg"], [("invalid boxes", boxes, 4, want)])
    for acc in (BVH, NAIVE):
        assert (got[acc, "invalid boxes", ALL]["tests"][bad] == 0).all()


# ---- 8. layouts, chunks, state and stream ------------------------------------------------------------------
def test_chunks_a_stride_of_six_and_permutations(soup0):
    import mobileraytracer_amd as m
    rng = np.random.default_rng(82)
    boxes = np.concatenate([soup0["boxes"], C.scene_boxes(soup0["geom"], 600, 83, 2.2), C.scene_boxes(soup0["geom"], 600, 84, 2.2),
                            soup0["boxes"][:200]])
    want = soup0["lists"].expected(boxes, 4)
    perm = rng.permutation(len(boxes))
    for acc in (BVH, NAIVE):
        with m.Renderer(dataclasses.replace(soup0["cfg"], accelerator=acc, maxPathsPerPass=512)) as r:
            cap = r.queue_info()["rayCap"][0]
            assert 64 <= cap and 3 * cap < len(boxes)  # several chunks, the last one partial or not
            rows = dev(boxes)  # an (n, 6) array read in place: mn and mx 6 floats apart
            assert rows[:, 3:].data_ptr() == rows.data_ptr() + 12
            got = {f: x.cpu().numpy() for f, x in r.overlap_boxes(rows[:, :3], rows[:, 3:], 4).items()}
            packed = {f: x.cpu().numpy() for f, x in r.overlap_boxes(dev(boxes[:, :3].copy()), dev(boxes[:, 3:].copy()), 4).items()}
            mixed = query(r, boxes[perm], 4)
        C.assert_same(got, want, "2000 boxes in chunks of %d, strides 6, accelerator %d" % (cap, acc))
        C.assert_same(packed, want, "packed, accelerator %d" % acc)
        C.assert_same(mixed, C.rows_of(want, perm), "permuted, accelerator %d" % acc)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches_and_single_fields_write_their_entries_and_nothing_else(soup0, n):
    import ctypes
    import torch
    import mobileraytracer_amd as m
    K, guard = 4, 64
    rows = slice(190, 190 + n)  # (points of the surface, then corners)
    want = C.rows_of(soup0["want"][K], rows)
    db = dev(soup0["boxes"][rows])
    size = {f: n * (1 if w == 0 else K * w) for f, w in C.WIDTHS.items()}

    def outputs():
        return {f: torch.full((guard + size[f] + guard,), SENTINEL, dtype=torch.int32, device="cuda") for f in ALL}

    def check(out, wanted, what):
        for f in ALL:
            x = out[f].cpu().numpy()
            assert (x[:guard] == SENTINEL).all() and (x[guard + size[f]:] == SENTINEL).all(), (what, f)
            body = x[guard:guard + size[f]]
            if f not in wanted:
                assert (body == SENTINEL).all(), (what, f)
            elif f != "tests":
                assert np.array_equal(body, want[f].reshape(-1)), (what, f)

    for acc in (BVH, NAIVE):
        with m.Renderer(dataclasses.replace(soup0["cfg"], accelerator=acc)) as r:
            for wanted in [ALL] + [(f,) for f in ALL]:
                out = outputs()
                torch.cuda.synchronize()  # (stream 0 is the renderer's own stream: not ordered after torch's fills)
                r.overlap_boxes_device(db.data_ptr(), db.data_ptr() + 12, n, K, mn_stride=6, mx_stride=6,
                                       **{"d_" + f: out[f][guard:].data_ptr() for f in wanted})
                torch.cuda.synchronize()
                check(out, wanted, (acc, wanted))
            # a smaller outSize: the cut-off fields count as NULL
            out = outputs()
            torch.cuda.synchronize()
            r.overlap_boxes_device(db.data_ptr(), db.data_ptr() + 12, n, K, mn_stride=6, mx_stride=6,
                                   out_size=3 * ctypes.sizeof(ctypes.c_void_p), **{"d_" + f: out[f][guard:].data_ptr() for f in ALL})
            torch.cuda.synchronize()
            check(out, ("any", "count", "kind"), (acc, "outSize 24"))


def test_a_query_leaves_frames_totals_and_other_queries_alone(tmp_path):
    import mobileraytracer_amd as m
    cfg = dataclasses.replace(NB.obj_cfg(S.write_base(str(tmp_path))), width=32, height=32)
    rng = np.random.default_rng(91)
    geom = m.scene_triangles(cfg)[0]
    boxes = C.scene_boxes(geom, 240, 92, 20.0)
    pts = np.concatenate([rng.uniform((-9, -6, -11), (9, 10, 4), (136, 3)), NB.surface_points(geom, 120, rng, 1e-3)]).astype(f32)
    want = C.Lists(cfg).expected(boxes, 4)
    o = np.stack([rng.uniform(-4, 4, 200), rng.uniform(-4, 4, 200), np.full(200, -9.0)], 1).astype(f32)
    d = np.stack([rng.uniform(-0.25, 0.25, 200), rng.uniform(-0.25, 0.25, 200), np.ones(200)], 1).astype(f32)

    def frame(r):
        bm = np.zeros(32 * 32, np.int32)
        r.render_frame(bm)
        st = r.frame_stats()
        return bm, r.frame_rays(), {k: v for k, v in st.items() if not k.endswith("Ms")}

    def others(r):
        cast = tuple(x.cpu().numpy() for x in r.cast_rays(dev(o), dev(d)))
        near = {f: x.cpu().numpy() for f, x in r.nearest_points(dev(pts)).items()}
        nb = {f: x.cpu().numpy() for f, x in r.neighbours(dev(pts), 4).items()}
        return cast, near, nb

    with m.Renderer(cfg) as plain:
        ref = [frame(plain), frame(plain)]
        ref_total = plain.get_total_casted_rays()
        ref_other = others(plain)
    with m.Renderer(cfg) as r:
        a = frame(r)
        total, stats = r.get_total_casted_rays(), r.frame_stats()
        bytes0 = r.scene_info()["deviceBytes"]
        got = query(r, boxes, 4)
        bytes1 = r.scene_info()["deviceBytes"]
        n_prims = sum(r.scene_info()[k] for k in ("triangles", "planes", "spheres"))
        assert 0 <= bytes1 - bytes0 <= 4 * n_prims + 4096  # the mapping tables, at the first query only
        before = others(r)
        again = query(r, boxes, 4, fields=("any",))
        after = others(r)
        assert r.scene_info()["deviceBytes"] == bytes1
        assert r.get_total_casted_rays() == total
        now = r.frame_stats()
        assert all(now[k] == stats[k] for k in stats if not k.endswith("Ms"))
        b = frame(r)
        assert r.get_total_casted_rays() == ref_total
    C.assert_same(got, want, "between two frames")
    C.assert_same(again, want, "again", fields=("any",))
    for cast, near, nb in (before, after):
        assert all(np.array_equal(bits(x) if x.dtype == f32 else x, bits(y) if y.dtype == f32 else y) for x, y in zip(cast, ref_other[0]))
        for x, y in ((near, ref_other[1]), (nb, ref_other[2])):
            assert set(x) == set(y)
            for f in x:
                assert np.array_equal(bits(x[f]) if x[f].dtype == f32 else x[f], bits(y[f]) if y[f].dtype == f32 else y[f]), f
    for x, y in ((a, ref[0]), (b, ref[1])):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2]
    assert a[1][0] > 0 and len(set(a[0].tolist())) > 1


def test_query_is_ordered_on_the_callers_stream(soup0):
    """On a stream of the caller's: a long run of kernels, then the kernel that fills the box tensor, then the
    query, then reductions of its outputs - and no synchronisation before the final copy.  A query that
    started before the fill would answer for boxes at the origin, a reduction that started before the query
    would read the sentinel."""
    import torch
    import mobileraytracer_amd as m
    K = 4
    n = len(soup0["boxes"])
    src_b = dev(soup0["boxes"])
    w = soup0["want"][K]
    want = [dev(x) for x in (w["count"], w["index"])]
    assert not np.array_equal(soup0["lists"].expected(np.zeros((1, 6), f32), K)["index"][0], w["index"][0])
    busy = torch.ones(1 << 24, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with m.Renderer(soup0["cfg"]) as r:
        with torch.cuda.stream(stream):
            b = torch.zeros(n, 6, device="cuda")
            c = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
            i = torch.full((n, K), SENTINEL, dtype=torch.int32, device="cuda")
            for _ in range(200):
                busy.mul_(1.0001)
            b.add_(src_b)
            r.overlap_boxes_device(b.data_ptr(), b.data_ptr() + 12, n, K, mn_stride=6, mx_stride=6, d_count=c.data_ptr(),
                                   d_index=i.data_ptr(), stream=stream.cuda_stream)
            wrong = (c != want[0]).sum() + (i != want[1]).sum()
            wrong = int(wrong.cpu())  # (the first wait for the device)
    assert wrong == 0


def test_regular_grid_and_device_groups_are_refused(soup0):
    import torch
    import mobileraytracer_amd as m
    db = dev(soup0["boxes"])
    n = len(soup0["boxes"])
    kind = torch.full((n, 4), SENTINEL, dtype=torch.int32, device="cuda")
    hit = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    for cfg, message in ((dataclasses.replace(soup0["cfg"], accelerator=GRID), "RegularGrid"),
                         (m.Config(width=16, height=16, shader=1, sceneIndex=0, devices=[0, 0]), "device groups are not supported")):
        with m.Renderer(cfg) as r:
            total = r.get_total_casted_rays()
            with pytest.raises(RuntimeError, match=message):
                r.overlap_boxes_device(db.data_ptr(), db.data_ptr() + 12, n, 4, mn_stride=6, mx_stride=6,
                                       d_kind=kind.data_ptr(), d_any=hit.data_ptr())
            with pytest.raises(RuntimeError, match=message):
                r.overlap_boxes_device(db.data_ptr(), db.data_ptr() + 12, n, 4, mn_stride=6, mx_stride=6, d_any=hit.data_ptr())
            with pytest.raises(RuntimeError, match=message):
                r.overlap_boxes(db[:, :3], db[:, 3:], 4)
            torch.cuda.synchronize()
            assert (kind.cpu().numpy() == SENTINEL).all() and (hit.cpu().numpy() == SENTINEL).all()
            assert r.get_total_casted_rays() == total


# ---- the wrappers --------------------------------------------------------------------------------------------
def test_wrapper_shapes_empty_batches_and_bad_fields(soup0):
    import torch
    import mobileraytracer_amd as m
    db = dev(soup0["boxes"][:70])
    with m.Renderer(soup0["cfg"]) as r:
        assert r.OVERLAP_FIELDS == ALL
        full = r.overlap_boxes(db[:, :3], db[:, 3:], 16)
        assert set(full) == set(ALL) and full["any"].shape == full["count"].shape == full["tests"].shape == (70,)
        assert full["kind"].shape == full["index"].shape == (70, 16) and full["kind"].dtype == torch.int32
        empty = r.overlap_boxes(db[:0, :3], db[:0, 3:], 4)
        assert set(empty) == set(ALL) and empty["count"].shape == (0,) and empty["kind"].shape == (0, 4)
        for bad in (("depth",), ()):
            with pytest.raises(ValueError):
                r.overlap_boxes(db[:, :3], db[:, 3:], 4, fields=bad)
        for k in (0, 17):
            with pytest.raises(ValueError):
                r.overlap_boxes(db[:, :3], db[:, 3:], k)
        with pytest.raises(TypeError):
            r.overlap_boxes_device(db.data_ptr(), db.data_ptr() + 12, 70, 4, d_normal=db.data_ptr())


def test_voxel_occupancy_shares_faces_between_cells(tmp_path):
    """A 4 x 4 sheet of unit quads in z = 0 under a lattice of 8 x 6 x 4 cells of 0.75 from (-1, -1, -1.5): the
    sheet lies in the shared face of the layers iz = 1 and iz = 2 (-1.5 + 0.75 * 2 = 0 exactly), so both layers
    hold it; the answer equals the host's on the same float32 cell bounds."""
    import mobileraytracer_amd as m
    cfg = NB.obj_cfg(NB.write_mesh(str(tmp_path), "sheet4", quads=NB.sheet_quads(4, 0), light=NB.FAR_LIGHT))
    origin, cell, dims = (-1.0, -1.0, -1.5), 0.75, (8, 6, 4)
    iz, iy, ix = np.meshgrid(np.arange(4), np.arange(6), np.arange(8), indexing="ij")
    idx = np.stack([ix, iy, iz], -1).reshape(-1, 3).astype(f32)
    o, c = np.array(origin, f32), f32(cell)
    boxes = np.concatenate([o + c * idx, o + c * (idx + f32(1))], 1)
    assert boxes.dtype == f32
    want = C.Lists(cfg).expected(boxes, 1)
    with m.Renderer(cfg) as r:
        occ = r.voxel_occupancy(origin, cell, dims).cpu().numpy()
        cnt = r.voxel_occupancy(origin, cell, dims, field="count").cpu().numpy()
        with pytest.raises(ValueError):
            r.voxel_occupancy(origin, cell, dims, field="kind")
    assert occ.shape == cnt.shape == (4, 6, 8) and occ.dtype == np.int32
    assert np.array_equal(occ.reshape(-1), want["any"]) and np.array_equal(cnt.reshape(-1), want["count"])
    assert occ[1].any() and np.array_equal(occ[1], occ[2]) and not occ[0].any() and not occ[3].any()
