"""Neighbour queries (mrt_neighbours_device): the K nearest surfaces to each point, in order, and the number
within the point's radius.  Every comparison is exact (count, kind, index, and the bits of dist2, point and
bary) against lists built on the host: mrt_point_distance on every candidate of the scene accessors, the
documented total order applied in NumPy (neighbour_cases.Lists).  Each case runs in both forms - `count`
wanted (the radius search) and not (the K-nearest search) - and under BVH and Naive unless it says
otherwise.  `tests` is diagnostic and compared nowhere, only bounded where the cull is the subject.

Frames are 16 x 16; outputs given to the C entry point start filled with a sentinel."""
import dataclasses

import numpy as np
import pytest

import nearest_cases as N
import neighbour_cases as C
import shape_scenes as S
from test_cast_rays_gpu import SENTINEL, bits, dev

pytestmark = pytest.mark.gpu

f32 = np.float32
NAIVE, GRID, BVH = 1, 2, 3
ALL = tuple(C.WIDTHS)
NO_COUNT = tuple(f for f in ALL if f != "count")


def query(r, points, k, max_dist=None, src=None, fields=None):
    got = r.neighbours(dev(points), k, max_dist=None if max_dist is None else dev(max_dist),
                       src=None if src is None else dev(src), fields=fields)
    return {f: x.cpu().numpy() for f, x in got.items()}


def both(cfg, jobs, accelerators=(BVH, NAIVE), entry0=False):
    """jobs: (what, points, k, keywords, want).  Each job under each accelerator, with `count` wanted and
    not: every answer equals the host's, so the accelerators and the two forms equal each other bit for
    bit.  entry0: entry 0 of every answer is also nearest_points' answer of the same renderer.  Returns the
    answers by (accelerator, what, count wanted)."""
    import mobileraytracer_amd as m
    out = {}
    for acc in accelerators:
        with m.Renderer(dataclasses.replace(cfg, accelerator=acc)) as r:
            for what, points, k, kw, want in jobs:
                for counted in (True, False):
                    got = query(r, points, k, fields=ALL if counted else NO_COUNT, **kw)
                    assert ("count" in got) == counted
                    name = "%s, K = %d, accelerator %d, count %s" % (what, k, acc, "wanted" if counted else "not wanted")
                    C.assert_same(got, want, name, fields=C.FIELDS if counted else C.LIST_FIELDS)
                    out[acc, what, counted] = got
                    if entry0:
                        one = r.nearest_points(dev(points), **{a: dev(b) for a, b in kw.items()})
                        N.assert_same({f: got[f][:, 0] for f in N.FIELDS}, {f: x.cpu().numpy() for f, x in one.items()},
                                      name + ", entry 0 against nearest_points")
    return out


# ---- 1. a soup: every field, K = 1, 4, 16, entry 0, truncation ---------------------------------------
def soup_case(path, offset, size, near):
    import mobileraytracer_amd as m
    cfg = C.obj_cfg(C.soup(path, "soup", offset, size))
    geom = m.scene_triangles(cfg)[0]
    assert len(geom) == 300
    pts = C.soup_points(geom, 200, near)
    lists = C.Lists(cfg)
    d2 = lists.distances(pts)
    case = {"cfg": cfg, "geom": geom, "pts": pts, "lists": lists, "d2": d2,
            "want": {k: lists.expected(pts, k, d2=d2) for k in (1, 4, 16)}}
    for x in (pts, d2):
        x.setflags(write=False)
    return case


@pytest.fixture(scope="module")
def soup0(tmp_path_factory):
    """The soup at the origin, 600 points (in a box twice the scene's, near the surface, on corners), their
    distances to all 302 candidates and the unbounded lists for K = 1, 4 and 16."""
    return soup_case(str(tmp_path_factory.mktemp("neighbour_soup")), 0.0, 0.2, 1e-3)


def check_soup(case, what):
    want = case["want"]
    assert (want[16]["count"] == 302).all() and (want[16]["kind"] == N.TRIANGLE).mean() > 0.9
    assert (want[16]["dist2"][:, 0] == 0).sum() >= 100  # (points on the surface: several candidates at 0)
    for k in (1, 4):  # (on the host: a shorter list is the longer one cut)
        C.assert_same(C.cut(want[16], k), want[k], "the host's own K = %d" % k)
    got = both(case["cfg"], [("%s, %d" % (what, k), case["pts"], k, {}, want[k]) for k in (1, 4, 16)], entry0=True)
    # truncation: count > K leaves the list equal to the first K of the K = 16 list
    for acc in (BVH, NAIVE):
        for counted in (True, False):
            long = got[acc, what + ", 16", counted]
            for k in (1, 4):
                short = got[acc, "%s, %d" % (what, k), counted]
                assert not counted or (short["count"] > k).all()
                C.assert_same(short, C.cut({f: long[f] for f in C.FIELDS if f in long}, k), "%s: K = %d against the K = 16 list" % (what, k))


def test_soup_at_the_origin(soup0):
    check_soup(soup0, "soup at 0")


def test_soup_at_1024(tmp_path):
    check_soup(soup_case(str(tmp_path), 1024.0, 0.01, 1e-4), "soup at 1024")


# ---- 2. radii ----------------------------------------------------------------------------------------
def test_radii_give_counts_of_0_1_k_minus_1_k_k_plus_1_and_all(soup0):
    """K = 4.  Each point's radius is chosen from the host's own sorted d2 - between the c-th and the
    (c + 1)-th accepted candidate for c = 0, 1, 3, 4, 5, or far beyond the scene - and 18 points get a radius
    of 0, below 0 or NaN.  With `count` wanted the walk must meet every candidate within the radius; without,
    the list must be the same."""
    K = 4
    pts, lists, d2 = soup0["pts"], soup0["lists"], soup0["d2"]
    n = len(pts)
    sd = np.sort(np.where(lists.valid[None, :], d2, np.inf).astype(np.float64), axis=1)
    classes = (0, 1, K - 1, K, K + 1, 302)
    radius = np.empty(n, f32)
    for i in range(n):
        c = classes[i % len(classes)]
        radius[i] = 1e6 if c == 302 else np.sqrt(sd[i, 0] / 2 if c == 0 else (sd[i, c - 1] + sd[i, c]) / 2)
    special = np.array([0.0, -1.0, np.nan, -np.inf, -0.0, -1e-30], f32)
    at = 31 * np.arange(18)  # (every class loses three points to them)
    radius[at] = np.tile(special, 3)
    want = lists.expected(pts, K, max_dist=radius, d2=d2)
    for c in classes:  # (on the host, before the GPU is asked)
        assert (want["count"] == c).sum() >= 16, (c, np.bincount(want["count"]))
    pad = want["count"][at]
    assert (pad == 0).all() and (want["kind"][at] == 0).all() and (want["index"][at] == -1).all()
    assert (bits(want["dist2"][at]) == 0).all() and (want["point"][at] == 0).all() and (want["bary"][at] == 0).all()
    got = both(soup0["cfg"], [("radii", pts, K, {"max_dist": radius}, want)], entry0=True)
    assert (got[NAIVE, "radii", True]["tests"] == 302).all()


# ---- 3. exact ties -----------------------------------------------------------------------------------
def test_exact_ties_are_listed_in_input_order(tmp_path):
    import mobileraytracer_amd as m
    cfg = C.obj_cfg(C.write_mesh(str(tmp_path), "sheets", quads=C.sheet_quads(16, 0) + C.sheet_quads(16, 2), light=C.FAR_LIGHT))
    geom = m.scene_triangles(cfg)[0]
    assert len(geom) == 1024
    lo = C.corners_of(geom).min(0)
    g = np.arange(33, dtype=f32) * f32(0.5)  # corners, edge midpoints and cell centres, midway between the sheets
    pts = np.stack([lo[0] + np.repeat(g, 33), lo[1] + np.tile(g, 33), np.full(33 * 33, lo[2] + 1, f32)], 1).astype(f32)
    lists = C.Lists(cfg)
    d2 = lists.distances(pts)
    ties = (d2[:, :1024] == 1.0).sum(1)
    assert (d2[:, :1024] >= 1.0).all() and (ties >= 2).all() and (ties >= 4).sum() >= 256
    want = {k: lists.expected(pts, k, d2=d2) for k in (4, 16)}
    # (on the host) the entries at d2 == 1.0 are those triangles in input order: the lowest indices first
    for i in np.nonzero(ties >= 4)[0][::16]:
        m16 = min(16, ties[i])
        assert np.array_equal(want[16]["index"][i, :m16], np.nonzero(d2[i, :1024] == 1.0)[0][:m16])
        assert (want[16]["kind"][i, :m16] == N.TRIANGLE).all()
    both(cfg, [("two sheets", pts, k, {}, want[k]) for k in (4, 16)], entry0=True)


# ---- 4. the other kinds ------------------------------------------------------------------------------
def test_planes_spheres_triangles_and_lights():
    import mobileraytracer_amd as m
    seen, point_lights = set(), 0
    for scene in (0, 1, 2, 3):
        cfg = m.Config(width=16, height=16, shader=1, sceneIndex=scene)
        lists = C.Lists(cfg)
        pts = C.builtin_points(lists.cands, 256, 60 + scene)
        want = lists.expected(pts, 4)
        kinds = {k: int((want["kind"] == k).sum()) for k in (1, 2, 3, 4)}
        print("scene %d: candidates %s, list entries per kind %s" % (scene, lists.cands.count, kinds))
        seen |= {k for k, c in kinds.items() if c >= 8}
        lkind = m.scene_lights(cfg)[0]
        point_lights += int((lkind == 0).sum())
        lit = want["kind"] == N.LIGHT
        assert (lkind[want["index"][lit]] == 1).all()  # a point light never appears
        both(cfg, [("scene %d" % scene, pts, 4, {}, want)], entry0=True)
        # an accelerator id that builds nothing: the area lights only
        lights = C.Lists(cfg, lights_only=True)
        want0 = lights.expected(pts, 4)
        assert set(np.unique(want0["kind"])) <= {0, N.LIGHT} and (want0["count"] == (lkind == 1).sum()).all()
        both(cfg, [("scene %d, no accelerator" % scene, pts, 4, {}, want0)], accelerators=(0,), entry0=True)
    assert seen == {1, 2, 3, 4} and point_lights >= 1


# ---- 5. the cull -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sheet(tmp_path_factory):
    """The 46 x 46 sheet of unit quads (4232 triangles, two far lights), 1024 points at height 0.5 above it,
    their distances and the K = 16 lists with a radius of 2 and with none."""
    import mobileraytracer_amd as m
    cfg = C.obj_cfg(C.write_mesh(str(tmp_path_factory.mktemp("neighbour_sheet")), "sheet46", quads=C.sheet_quads(46, 0),
                                 light=C.FAR_LIGHT))
    geom = m.scene_triangles(cfg)[0]
    T = len(geom)
    assert T == 4232
    lo = C.corners_of(geom).min(0)
    rng = np.random.default_rng(41)
    pts = np.concatenate([lo[:2] + rng.integers(0, 46, (1024, 2)) + rng.random((1024, 2)), np.full((1024, 1), lo[2] + 0.5)], 1).astype(f32)
    lists = C.Lists(cfg)
    assert lists.fixed == 2
    d2 = lists.distances(pts)
    radius = np.full(1024, 2.0, f32)
    return {"cfg": cfg, "T": T, "F": lists.fixed, "pts": pts, "lists": lists, "d2": d2, "radius": radius,
            "near": lists.expected(pts, 16, max_dist=radius, d2=d2), "free": lists.expected(pts, 16, d2=d2)}


def test_the_radius_form_meets_what_lies_within_the_radius_and_little_more(sheet):
    """`count` wanted, radius 2.  The bound on `tests` comes from the tree, not from the walk: a triangle
    can only be evaluated if its leaf's box is within the threshold, thr = (sqrt(bound2) + 2 c1)^2 (1 + 2^-20)
    with c1 = 32 * 2^-24 * Mq, here computed in float64 with a relative slack of 1e-4 (the float32 roundings
    of lb and thr are a few 2^-24)."""
    import mobileraytracer_amd as m
    T, F, pts, want = sheet["T"], sheet["F"], sheet["pts"], sheet["near"]
    assert (want["count"] > 16).mean() > 0.9  # (fewer at the sheet's rim)
    assert np.isin(want["kind"], (0, N.TRIANGLE)).all()  # (the lights are out of reach)
    boxes, _, cnt, _ = m.triangle_bvh(sheet["cfg"])
    leaf = cnt > 0
    assert cnt[leaf].sum() == T
    b, p = boxes[leaf].astype(np.float64), pts.astype(np.float64)
    gap = np.maximum(np.maximum(b[None, :, :3] - p[:, None, :], p[:, None, :] - b[None, :, 3:]), 0.0)
    lb = (gap * gap).sum(2)
    Mq = np.maximum(np.abs(p).max(1), np.abs(boxes[0].astype(np.float64)).max())
    thr = (2.0 + 2 * N.K_KERNEL * N.EPS * Mq) ** 2 * (1 + 2.0 ** -20) * (1 + 1e-4)
    reach = ((lb <= thr[:, None]) * cnt[leaf][None, :]).sum(1)
    got = both(sheet["cfg"], [("sheet, radius 2", pts, 16, {"max_dist": sheet["radius"]}, want)])
    assert (got[NAIVE, "sheet, radius 2", True]["tests"] == T + F).all()
    tests = got[BVH, "sheet, radius 2", True]["tests"]
    print("46 x 46 sheet, radius 2, count wanted: mean count %.1f, mean tests per point %.1f, mean triangles in reach "
          "of the threshold %.1f (of %d)" % (want["count"].mean(), tests.mean(), reach.mean(), T))
    assert (want["count"] <= tests - F).all() and (tests - F <= reach).all()
    assert reach.mean() < T / 8  # (the bound says something)


def test_the_k_nearest_form_skips_most_of_a_sheet(sheet):
    """`count` not wanted, no radius, K = 16: at least the 16 entries and the fixed candidates are
    evaluated, and on average fewer than an eighth of the triangles (the cap test_nearest_gpu.py holds K = 1
    to on this sheet).  Measured on an MI355X: 33.7 tests per point at K = 16, 5.9 at K = 1."""
    import mobileraytracer_amd as m
    T, F, pts, want = sheet["T"], sheet["F"], sheet["pts"], sheet["free"]
    assert (want["count"] == T + F).all()
    with m.Renderer(dataclasses.replace(sheet["cfg"], accelerator=BVH)) as r:
        got = query(r, pts, 16, fields=NO_COUNT)
        one = query(r, pts, 1, fields=NO_COUNT)
        counted = query(r, pts, 16, fields=ALL)
    C.assert_same(got, want, "sheet, K nearest", fields=C.LIST_FIELDS)
    C.assert_same(counted, want, "sheet, every candidate counted")
    assert (counted["tests"] == T + F).all()  # (count wanted and no radius: nothing may be skipped)
    mean = got["tests"].mean()
    print("46 x 46 sheet, K nearest: %d triangles, mean tests per point %.1f at K = 16, %.1f at K = 1" % (T, mean, one["tests"].mean()))
    assert (got["tests"] >= 16 + F).all() and mean < T / 8


# ---- 6. tree shapes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack%d" % S.STACK_DEEP, "degenerate", "inf_vertex", "outlier"])
def test_tree_shapes(tmp_path, name):
    import mobileraytracer_amd as m
    files = S.write_scene(str(tmp_path), name)
    cfg = C.obj_cfg(files[:3])
    if name.startswith("stack"):
        assert m.walk_stack(cfg)["need"] == S.STACK_CASES[S.STACK_DEEP][1]  # far beyond the LDS stack
    rng = np.random.default_rng(51)
    geom = m.scene_triangles(cfg)[0]
    pts = np.concatenate([rng.uniform((-9, -13, -11), (9, 10, 41), (32, 3)), C.surface_points(geom, 24, rng, 1e-3),
                          C.corner_points(geom, 24, rng)]).astype(f32)
    pts = pts[np.isfinite(pts).all(1)][:64]
    assert len(pts) == 64
    lists = C.Lists(cfg)
    d2 = lists.distances(pts)
    if name == "inf_vertex":
        assert np.isnan(d2).any()  # (left out of the lists and the counts)
    want = lists.expected(pts, 4, d2=d2)
    assert not np.isnan(want["dist2"]).any() and (want["count"] >= 4).all()
    assert (want["count"] == (~np.isnan(d2) & lists.valid[None, :]).sum(1)).all()
    both(cfg, [(name, pts, 4, {}, want)], entry0=True)


# ---- 7. sources --------------------------------------------------------------------------------------
def test_a_source_triangle_leaves_the_list_and_the_count(soup0):
    lists, geom = soup0["lists"], soup0["geom"]
    rng = np.random.default_rng(73)
    n = 200
    j = rng.integers(0, len(geom), n)
    w = np.array([(0.25, 0.25), (0.5, 0.25), (0.125, 0.5)], f32)[rng.integers(0, 3, n)]
    t = geom.reshape(-1, 9)[j]
    pts = ((t[:, :3] + t[:, 3:6] * w[:, :1]) + t[:, 6:] * w[:, 1:]).astype(f32)  # on or next to triangle j
    d2 = lists.distances(pts)
    radius = np.full(n, 0.5, f32)
    free = lists.expected(pts, 4, max_dist=radius, d2=d2)
    assert ((free["kind"][:, 0] == N.TRIANGLE) & (free["index"][:, 0] == j)).mean() > 0.9
    src = np.stack([np.full(n, N.TRIANGLE), j], 1).astype(np.int32)
    want = lists.expected(pts, 4, max_dist=radius, src=src, d2=d2)
    assert (want["count"] == free["count"] - 1).all() and (want["count"] >= 1).mean() > 0.9
    assert not ((want["kind"] == N.TRIANGLE) & (want["index"] == j[:, None])).any()
    both(soup0["cfg"], [("source triangles", pts, 4, {"max_dist": radius, "src": src}, want)], entry0=True)
    # a sphere or light source, a kind that is none, an index out of range: no source
    jobs = [("src %s" % (pair,), pts, 4, {"max_dist": radius, "src": np.tile(np.array([pair], np.int32), (n, 1))}, free)
            for pair in ((N.SPHERE, 0), (N.LIGHT, 0), (N.LIGHT, 1), (N.TRIANGLE, 300), (N.TRIANGLE, 1 << 20), (N.TRIANGLE, -1),
                         (N.PLANE, 0), (7, 0), (0, 0))]
    both(soup0["cfg"], jobs, accelerators=(BVH,))


def test_a_source_plane_leaves_the_list_and_the_count():
    import mobileraytracer_amd as m
    cfg = next(c for c in (m.Config(width=16, height=16, shader=1, sceneIndex=s) for s in (0, 1, 2, 3))
               if len(m.scene_planes(c)[0]) >= 2)
    lists = C.Lists(cfg)
    pts = C.builtin_points(lists.cands, 128, 74)
    d2 = lists.distances(pts)
    P = len(lists.rec[N.PLANE])
    j = np.argmin(d2[:, lists.first[N.PLANE]:lists.first[N.PLANE] + P], 1)  # each point's nearest plane
    free = lists.expected(pts, 4, d2=d2)
    assert ((free["kind"] == N.PLANE) & (free["index"] == j[:, None])).any(1).sum() >= 32
    src = np.stack([np.full(len(pts), N.PLANE), j], 1).astype(np.int32)
    want = lists.expected(pts, 4, src=src, d2=d2)
    assert (want["count"] == free["count"] - 1).all()
    assert not ((want["kind"] == N.PLANE) & (want["index"] == j[:, None])).any()
    both(cfg, [("source planes", pts, 4, {"src": src}, want)], entry0=True)
    both(cfg, [("plane %d of %d" % (P, P), pts, 4, {"src": np.tile(np.array([(N.PLANE, P)], np.int32), (len(pts), 1))}, free)],
         accelerators=(BVH,))


# ---- 8. chunks and layout ----------------------------------------------------------------------------
def test_chunks_and_a_stride_of_six(soup0):
    import mobileraytracer_amd as m
    pts = C.soup_points(soup0["geom"], 667, 1e-3, seed=82)[:2000]
    want = soup0["lists"].expected(pts, 4)
    wide = np.concatenate([pts, np.full((len(pts), 3), 7.0, f32)], 1)
    for acc in (BVH, NAIVE):
        with m.Renderer(dataclasses.replace(soup0["cfg"], accelerator=acc, maxPathsPerPass=512)) as r:
            cap = r.queue_info()["rayCap"][0]
            assert 64 <= cap and 3 * cap < len(pts)  # several chunks, the last one partial or not
            got = query(r, pts, 4)
            rows = dev(wide)
            strided = {f: x.cpu().numpy() for f, x in r.neighbours(rows[:, :3], 4).items()}  # read in place: rows 6 floats apart
        C.assert_same(got, want, "2000 points in chunks of %d, accelerator %d" % (cap, acc))
        C.assert_same(strided, want, "stride 6, accelerator %d" % acc)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches_and_single_fields_write_their_entries_and_nothing_else(soup0, n):
    import ctypes
    import torch
    import mobileraytracer_amd as m
    K, guard = 4, 64
    want = C.rows_of(soup0["want"][K], slice(0, n))
    dp = dev(soup0["pts"][:n])
    size = {f: n * (1 if w == 0 else K * w) for f, w in C.WIDTHS.items()}

    def outputs():
        return {f: torch.full((guard + size[f] + guard,), SENTINEL, dtype=torch.int32, device="cuda") for f in ALL}

    def check(out, wanted, what):
        res = {}
        for f in ALL:
            x = out[f].cpu().numpy()
            assert (x[:guard] == SENTINEL).all() and (x[guard + size[f]:] == SENTINEL).all(), (what, f)
            body = x[guard:guard + size[f]]
            if f not in wanted:
                assert (body == SENTINEL).all(), (what, f)
            elif f != "tests":
                e = want[f] if want[f].dtype == np.int32 else bits(want[f])
                assert np.array_equal(body, e.reshape(-1)), (what, f)
            res[f] = body
        return res

    for acc in (BVH, NAIVE):
        with m.Renderer(dataclasses.replace(soup0["cfg"], accelerator=acc)) as r:
            for wanted in [ALL] + [(f,) for f in ALL]:
                out = outputs()
                torch.cuda.synchronize()  # (stream 0 is the renderer's own stream: not ordered after torch's fills)
                r.neighbours_device(dp.data_ptr(), n, K, **{"d_" + f: out[f][guard:].data_ptr() for f in wanted})
                torch.cuda.synchronize()
                res = check(out, wanted, (acc, wanted))
                if "tests" in wanted:
                    assert (res["tests"] >= K).all()
            # a smaller outSize: the cut-off fields count as NULL
            out = outputs()
            torch.cuda.synchronize()
            r.neighbours_device(dp.data_ptr(), n, K, out_size=4 * ctypes.sizeof(ctypes.c_void_p),
                                **{"d_" + f: out[f][guard:].data_ptr() for f in ALL})
            torch.cuda.synchronize()
            check(out, ("count", "kind", "index", "dist2"), (acc, "outSize 32"))


# ---- 9. state ----------------------------------------------------------------------------------------
def test_a_query_leaves_frames_totals_and_other_queries_alone(tmp_path):
    import mobileraytracer_amd as m
    cfg = dataclasses.replace(C.obj_cfg(S.write_base(str(tmp_path))), width=32, height=32)
    rng = np.random.default_rng(91)
    geom = m.scene_triangles(cfg)[0]
    pts = np.concatenate([rng.uniform((-9, -6, -11), (9, 10, 4), (136, 3)), C.surface_points(geom, 120, rng, 1e-3)]).astype(f32)
    want = C.Lists(cfg).expected(pts, 4)
    o = np.stack([rng.uniform(-4, 4, 200), rng.uniform(-4, 4, 200), np.full(200, -9.0)], 1).astype(f32)
    d = np.stack([rng.uniform(-0.25, 0.25, 200), rng.uniform(-0.25, 0.25, 200), np.ones(200)], 1).astype(f32)

    def frame(r):
        bm = np.zeros(32 * 32, np.int32)
        r.render_frame(bm)
        st = r.frame_stats()
        return bm, r.frame_rays(), {k: v for k, v in st.items() if not k.endswith("Ms")}

    def cast(r):
        return tuple(x.cpu().numpy() for x in r.cast_rays(dev(o), dev(d)))

    def nearest(r):
        return {f: x.cpu().numpy() for f, x in r.nearest_points(dev(pts)).items()}

    with m.Renderer(cfg) as plain:
        ref = [frame(plain), frame(plain)]
        ref_total = plain.get_total_casted_rays()
        ref_cast = cast(plain)
        ref_near = nearest(plain)
    with m.Renderer(cfg) as r:
        a = frame(r)
        total, stats = r.get_total_casted_rays(), r.frame_stats()
        bytes0 = r.scene_info()["deviceBytes"]
        got = query(r, pts, 4)
        bytes1 = r.scene_info()["deviceBytes"]
        n_prims = sum(r.scene_info()[k] for k in ("triangles", "planes", "spheres"))
        assert 0 <= bytes1 - bytes0 <= 4 * n_prims + 4096  # the mapping tables, at the first query only
        before = cast(r), nearest(r)
        again = query(r, pts, 4, fields=("kind", "dist2"))
        after = cast(r), nearest(r)
        assert r.scene_info()["deviceBytes"] == bytes1
        assert r.get_total_casted_rays() == total
        now = r.frame_stats()
        assert all(now[k] == stats[k] for k in stats if not k.endswith("Ms"))
        b = frame(r)
        assert r.get_total_casted_rays() == ref_total
    C.assert_same(got, want, "between two frames")
    C.assert_same(again, want, "again", fields=("kind", "dist2"))
    for q, near in (before, after):
        assert np.array_equal(q[0], ref_cast[0]) and np.array_equal(q[1], ref_cast[1]) and np.array_equal(bits(q[2]), bits(ref_cast[2]))
        N.assert_same(near, ref_near, "nearest_points")
        assert np.array_equal(near["tests"], ref_near["tests"])
    assert (ref_cast[0] > 0).mean() > 0.5
    for x, y in ((a, ref[0]), (b, ref[1])):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2]
    assert a[1][0] > 0 and len(set(a[0].tolist())) > 1


def test_query_is_ordered_on_the_callers_stream(soup0):
    """On a stream of the caller's: a long run of kernels, then the kernel that fills the point tensor, then
    the query, then reductions of its outputs - and no synchronisation before the final copies.  A query
    that started before the fill would answer for the origin, a reduction that started before the query
    would read the sentinel."""
    import torch
    import mobileraytracer_amd as m
    K = 4
    n = len(soup0["pts"])
    src_p = dev(soup0["pts"])
    w = soup0["want"][K]
    want = [dev(x) for x in (w["count"], w["index"], bits(w["dist2"]))]
    assert not np.array_equal(soup0["lists"].expected(np.zeros((1, 3), f32), K)["index"][0], w["index"][0])
    busy = torch.ones(1 << 24, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with m.Renderer(soup0["cfg"]) as r:
        with torch.cuda.stream(stream):
            p = torch.zeros(n, 3, device="cuda")
            c = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
            i = torch.full((n, K), SENTINEL, dtype=torch.int32, device="cuda")
            t = torch.full((n, K), SENTINEL, dtype=torch.int32, device="cuda")
            for _ in range(200):
                busy.mul_(1.0001)
            p.add_(src_p)
            r.neighbours_device(p.data_ptr(), n, K, d_count=c.data_ptr(), d_index=i.data_ptr(), d_dist2=t.data_ptr(),
                                stream=stream.cuda_stream)
            wrong = (c != want[0]).sum() + (i != want[1]).sum() + (t != want[2]).sum()
            wrong = int(wrong.cpu())  # (the first wait for the device)
    assert wrong == 0


# ---- 10. refusals ------------------------------------------------------------------------------------
def test_regular_grid_and_device_groups_are_refused(soup0):
    import torch
    import mobileraytracer_amd as m
    dp = dev(soup0["pts"])
    n = len(soup0["pts"])
    kind = torch.full((n, 4), SENTINEL, dtype=torch.int32, device="cuda")
    count = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    for cfg, message in ((dataclasses.replace(soup0["cfg"], accelerator=GRID), "RegularGrid"),
                         (m.Config(width=16, height=16, shader=1, sceneIndex=0, devices=[0, 0]), "device groups are not supported")):
        with m.Renderer(cfg) as r:
            total = r.get_total_casted_rays()
            with pytest.raises(RuntimeError, match=message):
                r.neighbours_device(dp.data_ptr(), n, 4, d_kind=kind.data_ptr(), d_count=count.data_ptr())
            with pytest.raises(RuntimeError, match=message):
                r.neighbours_device(dp.data_ptr(), n, 4, d_kind=kind.data_ptr())
            with pytest.raises(RuntimeError, match=message):
                r.neighbours(dp, 4)
            torch.cuda.synchronize()
            assert (kind.cpu().numpy() == SENTINEL).all() and (count.cpu().numpy() == SENTINEL).all()
            assert r.get_total_casted_rays() == total


# ---- the wrapper -------------------------------------------------------------------------------------
def test_wrapper_shapes_empty_batches_and_bad_fields(soup0):
    import torch
    import mobileraytracer_amd as m
    dp = dev(soup0["pts"][:70])
    with m.Renderer(soup0["cfg"]) as r:
        assert r.NEIGHBOUR_FIELDS == ALL
        full = r.neighbours(dp, 16)
        assert set(full) == set(ALL) and full["count"].shape == (70,) and full["tests"].shape == (70,)
        assert full["kind"].shape == full["index"].shape == full["dist2"].shape == (70, 16)
        assert full["point"].shape == (70, 16, 3) and full["bary"].shape == (70, 16, 2)
        empty = r.neighbours(dp[:0], 4)
        assert set(empty) == set(ALL) and empty["count"].shape == (0,) and empty["kind"].shape == (0, 4)
        assert empty["point"].shape == (0, 4, 3) and empty["bary"].shape == (0, 4, 2)
        assert empty["kind"].dtype == torch.int32 and empty["dist2"].dtype == torch.float32
        only = r.neighbours(dp, 4, fields=("dist2", "point"))
        assert set(only) == {"dist2", "point"} and only["point"].shape == (70, 4, 3)
        C.assert_same({f: x.cpu().numpy() for f, x in only.items()}, C.rows_of(soup0["want"][4], slice(0, 70)),
                      "two fields", fields=("dist2", "point"))
        for bad in (("depth",), ()):
            with pytest.raises(ValueError):
                r.neighbours(dp, 4, fields=bad)
        for k in (0, 17):
            with pytest.raises(ValueError):
                r.neighbours(dp, k)
        with pytest.raises(TypeError):
            r.neighbours_device(dp.data_ptr(), 70, 4, d_normal=dp.data_ptr())
