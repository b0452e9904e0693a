"""Triangle overlap queries (mrt_overlap_triangles_device): the surfaces each query triangle touches, in (kind,
input index) order, and their number.  Every comparison is exact on ints against lists built on the host:
mrt_triangle_overlap on every candidate of the scene accessors, the documented order applied in NumPy
(triangle_overlap_cases.Lists).  Each case runs with three field sets - all fields, `count` only, `any` only (the
form that stops at the first acceptance) - and under BVH and Naive unless it says otherwise, so the two agree
bit for bit in every field but `tests`, which is diagnostic and only bounded where the cull is the subject.

Frames are 16 x 16; outputs given to the C entry point start filled with a sentinel."""
import dataclasses

import numpy as np
import pytest

import neighbour_cases as NB
import shape_scenes as S
import triangle_overlap_cases as T
from test_cast_rays_gpu import SENTINEL, bits, dev

pytestmark = pytest.mark.gpu

f32 = np.float32
NAIVE, GRID, BVH = 1, 2, 3
ALL = tuple(T.WIDTHS)
COUNT = ("count", "tests")
ANY = ("any", "tests")  # (`tests` does not change the form)
FORMS = (ALL, COUNT, ANY)


def query(r, tris, k, fields=None):
    got = r.overlap_triangles(dev(np.ascontiguousarray(tris, f32).reshape(-1, 9)), k, fields=fields)
    return {f: x.cpu().numpy() for f, x in got.items()}


def every_form(cfg, jobs, accelerators=(BVH, NAIVE)):
    """jobs: (what, triangles, k, want).  Each job under each accelerator with each field set: every answer equals
    the host's, so the accelerators and the forms equal each other bit for bit.  Returns the answers by
    (accelerator, what, field set)."""
    import mobileraytracer_amd as m
    out = {}
    for acc in accelerators:
        with m.Renderer(dataclasses.replace(cfg, accelerator=acc)) as r:
            for what, tris, k, want in jobs:
                for fields in FORMS:
                    got = query(r, tris, k, fields=fields)
                    assert set(got) == set(fields)
                    T.assert_same(got, want, "%s, K = %d, accelerator %d, fields %s" % (what, k, acc, fields))
                    if "count" in got and "any" in got:
                        assert np.array_equal(got["any"], (got["count"] > 0).astype(np.int32))
                    out[acc, what, fields] = got
    return out


# ---- 1. the device's functions are the host's ---------------------------------------------------------
KAT = {T.PLANE: [lambda n: T.plane_pairs(n, 211)], T.SPHERE: [lambda n: T.sphere_pairs(n, 212)],
       T.TRIANGLE: [lambda n: T.contract_pairs(n, 213, 0.0), lambda n: T.contract_pairs(n, 214, 4096.0),
                    lambda n: T.coplanar_pairs(n, 215), lambda n: T.shared_pairs(n, 216, 1),
                    lambda n: T.shared_pairs(n, 217, 2), lambda n: T.segment_pairs(n, 218),
                    lambda n: T.point_pairs(n, 219), lambda n: T.degenerate_pairs(n, 220)]}
KAT[T.LIGHT] = KAT[T.TRIANGLE]


@pytest.mark.parametrize("kind", [T.PLANE, T.SPHERE, T.TRIANGLE, T.LIGHT])
def test_kat_triangle_overlap_is_triangle_overlap(kind):
    import mobileraytracer_amd as m
    parts = [make((1 << 16) // len(KAT[kind])) for make in KAT[kind]]
    prims, tris = np.concatenate([p for p, _ in parts]), np.concatenate([t for _, t in parts])
    tris[::97, 3] = np.nan  # (and some invalid queries)
    tris[5::101, 7] = np.inf
    host = m.triangle_overlap(kind, prims, tris)
    assert 0.05 < host.mean() < 0.7 and (host[::97] == 0).all() and (host[5::101] == 0).all()
    assert np.array_equal(m.kat_triangle_overlap(kind, prims, tris), host)


# ---- 2. a soup: every field, K = 1, 4, 16, truncation ---------------------------------------------------
def soup_case(path, offset, size):
    import mobileraytracer_amd as m
    cfg = NB.obj_cfg(NB.soup(path, "soup", offset, size))
    geom = m.scene_triangles(cfg)[0]
    assert len(geom) == 300
    tris = T.scene_queries(geom, 600, 33, 1.0 + 6 * size)
    lists = T.Lists(cfg)
    ok = lists.accepted(tris)
    case = {"cfg": cfg, "geom": geom, "tris": tris, "lists": lists, "ok": ok,
            "want": {k: lists.expected(tris, k, ok=ok) for k in (1, 4, 16)}}
    for x in (tris, ok):
        x.setflags(write=False)
    return case


@pytest.fixture(scope="module")
def soup0(tmp_path_factory):
    """The soup at the origin, 600 query triangles (points, segments, triangles of every size, the scene's own
    triangles, one across the whole scene), the host's verdict on all 302 candidates and the lists for K = 1, 4
    and 16."""
    return soup_case(str(tmp_path_factory.mktemp("triangle_overlap_soup")), 0.0, 0.2)


def check_soup(case, what):
    want = case["want"]
    count = want[16]["count"]
    assert (count[:100] >= 1).mean() > 0.95 and (count[400:500] >= 1).all()  # (points of the surface; the scene's own)
    assert (count == 0).sum() >= 20 and (count > 16).sum() >= 20 and ((count > 0) & (count < 16)).sum() >= 100
    for k in (1, 4):  # (on the host: a shorter list is the longer one cut)
        T.assert_same(T.cut(want[16], k), want[k], "the host's own K = %d" % k)
    got = every_form(case["cfg"], [("%s, %d" % (what, k), case["tris"], k, want[k]) for k in (1, 4, 16)])
    for acc in (BVH, NAIVE):
        long = got[acc, what + ", 16", ALL]
        for k in (1, 4):
            T.assert_same(got[acc, "%s, %d" % (what, k), ALL], T.cut(long, k), "%s: K = %d against the K = 16 list" % (what, k))
    assert (got[NAIVE, what + ", 16", ALL]["tests"] == 302).all()


def test_soup_at_the_origin(soup0):
    check_soup(soup0, "soup at 0")


def test_soup_at_1024(tmp_path):
    check_soup(soup_case(str(tmp_path), 1024.0, 0.2), "soup at 1024")


# ---- 3. counts of 0, 1, K - 1, K, K + 1 and a whole sheet, coplanar ----------------------------------------
def test_counts_around_k_on_two_sheets(tmp_path):
    """Two 16 x 16 sheets of unit quads (z = 0 and z = 2).  Query triangles LYING IN the lower sheet - the
    coplanar path, where only the in-plane edge normals separate - placed against the cells' diagonals for
    counts of 1, K - 1, K, K + 1 and the whole sheet (K = 4); one between the sheets for 0.  Asserted on the host
    first."""
    import mobileraytracer_amd as m
    K = 4
    cfg = NB.obj_cfg(NB.write_mesh(str(tmp_path), "sheets", quads=NB.sheet_quads(16, 0) + NB.sheet_quads(16, 2), light=NB.FAR_LIGHT))
    geom = m.scene_triangles(cfg)[0]
    assert len(geom) == 1024
    lists = T.Lists(cfg)
    lo = NB.corners_of(geom).min(0).astype(np.float64)
    z = lo[2]
    rng = np.random.default_rng(35)
    rows = []
    for i in range(96):
        x, y = lo[:2] + rng.integers(1, 12, 2)
        c = i % 6
        if c == 0:    # between the sheets
            rows.append((x + 0.1, y + 0.1, z + 1, x + 3.9, y + 0.1, z + 1, x + 0.1, y + 3.9, z + 1))
        elif c == 1:  # inside a cell's lower-right triangle (the loaded quads are cut along y = x from the cell's corner)
            rows.append((x + 0.6, y + 0.1, z, x + 0.9, y + 0.1, z, x + 0.9, y + 0.3, z))
        elif c == 2:  # both triangles of one cell and the upper-left one of the next: 3
            rows.append((x + 0.6, y + 0.6, z, x + 1.4, y + 0.75, z, x + 0.6, y + 0.9, z))
        elif c == 3:  # both triangles of two cells: 4
            rows.append((x + 0.3, y + 0.45, z, x + 1.7, y + 0.5, z, x + 0.3, y + 0.55, z))
        elif c == 4:  # two, two and one: 5
            rows.append((x + 0.6, y + 0.6, z, x + 2.4, y + 0.75, z, x + 0.6, y + 0.9, z))
        else:         # the whole lower sheet and nothing of the upper one
            rows.append((lo[0] - 1, lo[1] - 1, z, lo[0] + 40, lo[1] - 1, z, lo[0] - 1, lo[1] + 40, z))
    tris = np.array(rows, f32)
    ok = lists.accepted(tris)
    want = lists.expected(tris, K, ok=ok)
    classes = (0, 1, K - 1, K, K + 1, 512)
    for c, cls in enumerate(classes):  # (on the host, before the GPU is asked)
        assert (want["count"][c::6] == cls).all(), (cls, want["count"][c::6])
    held = np.arange(K)[None, :] < want["count"][:, None]
    assert (want["kind"][~held] == 0).all() and (want["index"][~held] == -1).all()
    full = want["count"] > K  # truncation: the K smallest input indices
    first = np.argsort(~ok[full], axis=1, kind="stable")[:, :K]
    assert np.array_equal(want["index"][full], lists.index[first]) and (np.diff(want["index"][full], axis=1) > 0).all()
    every_form(cfg, [("sheets", tris, K, want)])


# ---- 4. the cull -----------------------------------------------------------------------------------------
def test_the_walk_tests_only_leaves_that_overlap_the_query_s_hull(tmp_path):
    """The 46 x 46 sheet: 1,024 small query triangles at the sheet, 64 above it that touch nothing.  `tests` is at
    most the triangles of the reference leaves whose boxes overlap the query's hull (closed compares on
    triangle_bvh's boxes) plus the lights; 0 triangles for a hull outside the root.  With `any` only no triangle
    costs more than in the full walk."""
    import mobileraytracer_amd as m
    cfg = NB.obj_cfg(NB.write_mesh(str(tmp_path), "sheet46", quads=NB.sheet_quads(46, 0), light=NB.FAR_LIGHT))
    geom = m.scene_triangles(cfg)[0]
    Tn = len(geom)
    assert Tn == 4232
    lo = NB.corners_of(geom).min(0)
    rng = np.random.default_rng(41)
    c = np.concatenate([lo[:2] + rng.integers(1, 45, (1024, 2)) + rng.random((1024, 2)), np.full((1024, 1), lo[2])], 1)
    h = 10.0 ** rng.uniform(-3, 0, (1024, 1, 1)) * 0.5
    off = rng.uniform(-1, 1, (1024, 3, 3))
    off[:, 0, 2], off[:, 1, 2] = np.abs(off[:, 0, 2]), -np.abs(off[:, 1, 2])  # (a corner on each side of the sheet)
    at = (c[:, None, :] + off * h).reshape(1024, 9).astype(f32)
    above = at[:64].copy()
    above[:, 2::3] = rng.uniform(lo[2] + 1, lo[2] + 2, (64, 3)).astype(f32)
    tris = np.concatenate([at, above])
    lists = T.Lists(cfg)
    want = lists.expected(tris, 16)
    assert (want["count"][:1024] >= 1).all() and (want["count"][1024:] == 0).all()
    nodes, _, cnt, _ = m.triangle_bvh(cfg)
    leaf = cnt > 0
    assert cnt[leaf].sum() == Tn
    b = nodes[leaf]
    hull = T.hull_of(tris)
    apart = ((b[None, :, :3] > hull[:, None, 3:]) | (b[None, :, 3:] < hull[:, None, :3])).any(2)
    reach = ((~apart) * cnt[leaf][None, :]).sum(1)
    got = every_form(cfg, [("sheet", tris, 16, want)])
    F = 2  # the two far lights, met one by one
    assert (got[NAIVE, "sheet", ALL]["tests"] == Tn + F).all()
    tests = got[BVH, "sheet", ALL]["tests"]
    fast = got[BVH, "sheet", ANY]["tests"]
    print("46 x 46 sheet: mean count %.1f, mean tests per triangle %.1f (any only: %.1f), mean triangles in overlapping "
          "leaves %.1f (of %d)" % (want["count"][:1024].mean(), tests.mean(), fast.mean(), reach.mean(), Tn))
    assert (want["count"] <= tests - F).all() and (tests - F <= reach).all()
    assert (tests[1024:] == F).all() and reach[:1024].mean() < Tn / 8
    assert (fast <= tests).all() and fast.mean() <= tests.mean()
    assert np.array_equal(got[BVH, "sheet", COUNT]["tests"], tests)  # (the counted form is the full walk)


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
    tris = T.scene_queries(fin, 60, 52, 20.0)
    big = [(-1e30, -1e30, -1e30, 1e30, 1e30, 1e30, 1e30, -1e30, 1e30), (-3e38, -3e38, -3e38, 3e38, 3e38, 3e38, 3e38, -3e38, 0),
           (-90, -130, -110, 90, 100, 410, 90, -130, 410), (0, 0, 0, 2.0 ** 41, 2.0 ** 41, 2.0 ** 41, 2.0 ** 41, 0, 2.0 ** 41)]
    tris = np.concatenate([tris, np.array(big, f32)]).astype(f32)
    lists = T.Lists(cfg)
    ok = lists.accepted(tris)
    want = lists.expected(tris, 4, ok=ok)
    bad = ~np.isfinite(lists.rec[T.TRIANGLE]).all(1)
    if name == "inf_vertex":
        assert bad.any()
    t0 = lists.first[T.TRIANGLE]
    assert not ok[:, t0:t0 + len(bad)][:, bad].any()  # a non-finite triangle is never accepted ...
    assert (want["count"] > 4).sum() >= 4 and (want["count"] == 0).sum() >= 1
    got = every_form(cfg, [(name, tris, 4, want)])
    big = every_form(cfg, [(name + ", 16", tris, 16, lists.expected(tris, 16, ok=ok))], accelerators=(BVH,))
    for res in list(got.values()) + list(big.values()):  # ... and never listed
        if "index" in res:
            assert not (np.isin(res["index"], np.nonzero(bad)[0]) & (res["kind"] == T.TRIANGLE)).any()


# ---- 6. other kinds ----------------------------------------------------------------------------------------
def test_planes_spheres_and_lights_and_no_accelerator():
    """Built-in scenes 1 - 3: query triangles about points near every kind's surfaces (found with point_distance),
    every seventh a point, and one triangle across everything: its list starts with the planes, then the spheres,
    the triangles, the lights.  With an accelerator id that builds nothing only the area lights are candidates."""
    import mobileraytracer_amd as m
    import nearest_cases as N
    seen = set()
    for scene in (1, 2, 3):
        cfg = m.Config(width=16, height=16, shader=1, sceneIndex=scene)
        lists = T.Lists(cfg)
        cands = N.Candidates(cfg)
        pts = NB.builtin_points(cands, 126, 60 + scene).astype(np.float64)
        rng = np.random.default_rng(61 + scene)
        h = 10.0 ** rng.uniform(-3, 0.5, (126, 1, 1)) * 0.5
        h[::7] = 0.0
        near = (pts[:, None, :] + rng.uniform(-1, 1, (126, 3, 3)) * h).reshape(126, 9)
        tris = np.concatenate([near, [(-1e4, -1e4, -1e4, 1e4, 1e4, 1e4, 1e4, -1e4, 1e4),
                                      (-1e4, -1e4, -1e4, -9e3, -9e3, -9e3, -9e3, -1e4, -9e3)]]).astype(f32)
        ok = lists.accepted(tris)
        want = lists.expected(tris, 16, ok=ok)
        kinds = {k: int((want["kind"] == k).sum()) for k in (1, 2, 3, 4)}
        print("scene %d: candidates %s, list entries per kind %s" % (scene, cands.count, kinds))
        seen |= {k for k, c in kinds.items() if c >= 4}
        lkind = m.scene_lights(cfg)[0]
        lit = want["kind"] == T.LIGHT
        assert (lkind[want["index"][lit]] == 1).all()  # a point light never appears
        for row in range(len(tris)):
            assert (np.diff(want["kind"][row][:min(want["count"][row], 16)]) >= 0).all()  # kind order
        every_form(cfg, [("scene %d" % scene, tris, 16, want), ("scene %d, 4" % scene, tris, 4, T.cut(want, 4))])
        lights = T.Lists(cfg, lights_only=True)
        want0 = lights.expected(tris, 4)
        assert set(np.unique(want0["kind"])) <= {0, T.LIGHT}
        every_form(cfg, [("scene %d, no accelerator" % scene, tris, 4, want0)], accelerators=(0,))
    assert seen == {1, 2, 3, 4}


# ---- 7. invalid, segment and point queries -------------------------------------------------------------------
def test_invalid_segment_and_point_queries_leave_their_neighbours_alone(soup0):
    tris = soup0["tris"][200:328].copy()  # (triangles about surface points)
    want = T.rows_of(soup0["want"][4], slice(200, 328))
    assert (want["count"] > 0).mean() > 0.5
    bad = np.arange(0, 128, 4)
    for i, row in enumerate(bad):
        tris[row, i % 9] = (np.nan, np.inf, -np.inf)[i % 3]
    seg = np.arange(1, 128, 4)
    tris[seg, 6:] = tris[seg, 3:6]
    pt = np.arange(2, 128, 4)
    tris[pt, 3:6] = tris[pt, :3]
    tris[pt, 6:] = tris[pt, :3]
    host = soup0["lists"].expected(tris, 4)
    keep = np.arange(3, 128, 4)
    T.assert_same(T.rows_of(host, keep), T.rows_of(want, keep), "the host's own answer for the rows left alone")
    assert (host["count"][bad] == 0).all() and (host["any"][bad] == 0).all() and (host["index"][bad] == -1).all()
    assert (host["kind"][bad] == 0).all() and (host["count"][seg] > 0).any() and (host["count"][seg] <= want["count"][seg]).all()
    got = every_form(soup0["cfg"], [("invalid, segment and point queries", tris, 4, host)])
    for acc in (BVH, NAIVE):
        tests = got[acc, "invalid, segment and point queries", ALL]["tests"]
        assert (tests[bad] == 0).all() and (tests[keep] > 0).all()


# ---- 8. layouts, chunks, state and stream ------------------------------------------------------------------
def test_chunks_a_stride_of_nine_and_permutations(soup0):
    import mobileraytracer_amd as m
    rng = np.random.default_rng(82)
    tris = np.concatenate([soup0["tris"], T.scene_queries(soup0["geom"], 600, 83, 2.2), T.scene_queries(soup0["geom"], 600, 84, 2.2),
                           soup0["tris"][:200]])
    want = soup0["lists"].expected(tris, 4)
    perm = rng.permutation(len(tris))
    for acc in (BVH, NAIVE):
        with m.Renderer(dataclasses.replace(soup0["cfg"], accelerator=acc, maxPathsPerPass=512)) as r:
            cap = r.queue_info()["rayCap"][0]
            assert 64 <= cap and 3 * cap < len(tris)  # several chunks, the last one partial or not
            rows = dev(tris)  # an (n, 9) array read in place: the corners 3 floats apart, the triangles 9
            out = {f: x.cpu().numpy() for f, x in r.overlap_triangles(rows, 4).items()}
            cube = {f: x.cpu().numpy() for f, x in r.overlap_triangles(rows.reshape(-1, 3, 3), 4).items()}
            wide = dev(np.concatenate([tris, np.full((len(tris), 3), np.nan, f32)], 1))  # rows 12 floats apart
            padded = {f: x.cpu().numpy() for f, x in r.overlap_triangles(wide[:, :9], 4).items()}
            a, b, c = (dev(tris[:, 3 * k:3 * k + 3].copy()) for k in range(3))  # three packed arrays
            sep = {f: np.full((len(tris),) if w == 0 else (len(tris), 4), SENTINEL, np.int32) for f, w in T.WIDTHS.items()}
            d_sep = {f: dev(x) for f, x in sep.items()}
            import torch
            torch.cuda.synchronize()
            r.overlap_triangles_device(a.data_ptr(), b.data_ptr(), c.data_ptr(), len(tris), 4,
                                       **{"d_" + f: x.data_ptr() for f, x in d_sep.items()})
            torch.cuda.synchronize()
            sep = {f: x.cpu().numpy() for f, x in d_sep.items()}
            mixed = query(r, tris[perm], 4)
        T.assert_same(out, want, "2000 triangles in chunks of %d, strides 9, accelerator %d" % (cap, acc))
        T.assert_same(cube, want, "(n, 3, 3), accelerator %d" % acc)
        T.assert_same(padded, want, "strides 12, accelerator %d" % acc)
        T.assert_same(sep, want, "three packed arrays, accelerator %d" % acc)
        T.assert_same(mixed, T.rows_of(want, perm), "permuted, accelerator %d" % acc)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches_and_single_fields_write_their_entries_and_nothing_else(soup0, n):
    import ctypes
    import torch
    import mobileraytracer_amd as m
    K, guard = 4, 64
    rows = slice(190, 190 + n)  # (segments, then triangles)
    want = T.rows_of(soup0["want"][K], rows)
    dt = dev(soup0["tris"][rows])
    size = {f: n * (1 if w == 0 else K * w) for f, w in T.WIDTHS.items()}
    p = dt.data_ptr()

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
                r.overlap_triangles_device(p, p + 12, p + 24, n, K, a_stride=9, b_stride=9, c_stride=9,
                                           **{"d_" + f: out[f][guard:].data_ptr() for f in wanted})
                torch.cuda.synchronize()
                check(out, wanted, (acc, wanted))
            # a smaller outSize: the cut-off fields count as NULL
            out = outputs()
            torch.cuda.synchronize()
            r.overlap_triangles_device(p, p + 12, p + 24, n, K, a_stride=9, b_stride=9, c_stride=9,
                                       out_size=3 * ctypes.sizeof(ctypes.c_void_p), **{"d_" + f: out[f][guard:].data_ptr() for f in ALL})
            torch.cuda.synchronize()
            check(out, ("any", "count", "kind"), (acc, "outSize 24"))


def test_a_query_leaves_frames_totals_and_other_queries_alone(tmp_path):
    import mobileraytracer_amd as m
    cfg = dataclasses.replace(NB.obj_cfg(S.write_base(str(tmp_path))), width=32, height=32)
    rng = np.random.default_rng(91)
    geom = m.scene_triangles(cfg)[0]
    tris = T.scene_queries(geom, 240, 92, 20.0)
    pts = np.concatenate([rng.uniform((-9, -6, -11), (9, 10, 4), (136, 3)), NB.surface_points(geom, 120, rng, 1e-3)]).astype(f32)
    want = T.Lists(cfg).expected(tris, 4)
    o = np.stack([rng.uniform(-4, 4, 200), rng.uniform(-4, 4, 200), np.full(200, -9.0)], 1).astype(f32)
    d = np.stack([rng.uniform(-0.25, 0.25, 200), rng.uniform(-0.25, 0.25, 200), np.ones(200)], 1).astype(f32)
    boxes = dev(T.hull_of(tris))

    def frame(r):
        bm = np.zeros(32 * 32, np.int32)
        r.render_frame(bm)
        st = r.frame_stats()
        return bm, r.frame_rays(), {k: v for k, v in st.items() if not k.endswith("Ms")}

    def others(r):
        cast = tuple(x.cpu().numpy() for x in r.cast_rays(dev(o), dev(d)))
        near = {f: x.cpu().numpy() for f, x in r.nearest_points(dev(pts)).items()}
        box = {f: x.cpu().numpy() for f, x in r.overlap_boxes(boxes[:, :3], boxes[:, 3:], 4).items() if f != "tests"}
        return cast, near, box

    with m.Renderer(cfg) as plain:
        ref = [frame(plain), frame(plain)]
        ref_total = plain.get_total_casted_rays()
        ref_other = others(plain)
    with m.Renderer(cfg) as r:
        a = frame(r)
        total, stats = r.get_total_casted_rays(), r.frame_stats()
        bytes0 = r.scene_info()["deviceBytes"]
        got = query(r, tris, 4)
        bytes1 = r.scene_info()["deviceBytes"]
        n_prims = sum(r.scene_info()[k] for k in ("triangles", "planes", "spheres"))
        assert 0 <= bytes1 - bytes0 <= 4 * n_prims + 4096  # the mapping tables, at the first query only
        before = others(r)
        again = query(r, tris, 4, fields=("any",))
        after = others(r)
        assert r.scene_info()["deviceBytes"] == bytes1  # no allocation after the first query
        assert r.get_total_casted_rays() == total
        now = r.frame_stats()
        assert all(now[k] == stats[k] for k in stats if not k.endswith("Ms"))
        b = frame(r)
        assert r.get_total_casted_rays() == ref_total
    T.assert_same(got, want, "between two frames")
    T.assert_same(again, want, "again", fields=("any",))
    for cast, near, box in (before, after):
        assert all(np.array_equal(bits(x) if x.dtype == f32 else x, bits(y) if y.dtype == f32 else y) for x, y in zip(cast, ref_other[0]))
        for x, y in ((near, ref_other[1]), (box, ref_other[2])):
            assert set(x) == set(y)
            for f in x:
                assert np.array_equal(bits(x[f]) if x[f].dtype == f32 else x[f], bits(y[f]) if y[f].dtype == f32 else y[f]), f
    for x, y in ((a, ref[0]), (b, ref[1])):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2]
    assert a[1][0] > 0 and len(set(a[0].tolist())) > 1


def test_query_is_ordered_on_the_callers_stream(soup0):
    """On a stream of the caller's: a long run of kernels, then the kernel that fills the triangle tensor, then
    the query, then reductions of its outputs - and no synchronisation before the final copy.  A query that
    started before the fill would answer for points at the origin, a reduction that started before the query
    would read the sentinel."""
    import torch
    import mobileraytracer_amd as m
    K = 4
    n = len(soup0["tris"])
    src = dev(soup0["tris"])
    w = soup0["want"][K]
    want = [dev(x) for x in (w["count"], w["index"])]
    at_origin = soup0["lists"].expected(np.zeros((1, 9), f32), K)["count"][0]
    assert (w["count"] != at_origin).mean() > 0.5  # (what a query that ran before the fill would answer)
    busy = torch.ones(1 << 24, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with m.Renderer(soup0["cfg"]) as r:
        with torch.cuda.stream(stream):
            t = torch.zeros(n, 9, device="cuda")
            c = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
            i = torch.full((n, K), SENTINEL, dtype=torch.int32, device="cuda")
            for _ in range(200):
                busy.mul_(1.0001)
            t.add_(src)
            p = t.data_ptr()
            r.overlap_triangles_device(p, p + 12, p + 24, n, K, a_stride=9, b_stride=9, c_stride=9, d_count=c.data_ptr(),
                                       d_index=i.data_ptr(), stream=stream.cuda_stream)
            wrong = (c != want[0]).sum() + (i != want[1]).sum()
            wrong = int(wrong.cpu())  # (the first wait for the device)
    assert wrong == 0


def test_regular_grid_and_device_groups_are_refused(soup0):
    import torch
    import mobileraytracer_amd as m
    dt = dev(soup0["tris"])
    n = len(soup0["tris"])
    p = dt.data_ptr()
    kind = torch.full((n, 4), SENTINEL, dtype=torch.int32, device="cuda")
    hit = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    for cfg, message in ((dataclasses.replace(soup0["cfg"], accelerator=GRID), "RegularGrid"),
                         (m.Config(width=16, height=16, shader=1, sceneIndex=0, devices=[0, 0]), "device groups are not supported")):
        with m.Renderer(cfg) as r:
            total = r.get_total_casted_rays()
            with pytest.raises(RuntimeError, match=message):
                r.overlap_triangles_device(p, p + 12, p + 24, n, 4, a_stride=9, b_stride=9, c_stride=9,
                                           d_kind=kind.data_ptr(), d_any=hit.data_ptr())
            with pytest.raises(RuntimeError, match=message):
                r.overlap_triangles_device(p, p + 12, p + 24, n, 4, a_stride=9, b_stride=9, c_stride=9, d_any=hit.data_ptr())
            with pytest.raises(RuntimeError, match=message):
                r.overlap_triangles(dt, 4)
            torch.cuda.synchronize()
            assert (kind.cpu().numpy() == SENTINEL).all() and (hit.cpu().numpy() == SENTINEL).all()
            assert r.get_total_casted_rays() == total


# ---- 13. the wrappers ----------------------------------------------------------------------------------------
def test_wrapper_shapes_empty_batches_and_bad_fields(soup0):
    import torch
    import mobileraytracer_amd as m
    dt = dev(soup0["tris"][:70])
    with m.Renderer(soup0["cfg"]) as r:
        full = r.overlap_triangles(dt, 16)
        assert set(full) == set(ALL) and full["any"].shape == full["count"].shape == full["tests"].shape == (70,)
        assert full["kind"].shape == full["index"].shape == (70, 16) and full["kind"].dtype == torch.int32
        for empty in (r.overlap_triangles(dt[:0], 4), r.overlap_triangles(dt[:0].reshape(0, 3, 3), 4)):
            assert set(empty) == set(ALL) and empty["count"].shape == (0,) and empty["kind"].shape == (0, 4)
        for bad in (("depth",), ()):
            with pytest.raises(ValueError):
                r.overlap_triangles(dt, 4, fields=bad)
        for k in (0, 17):
            with pytest.raises(ValueError):
                r.overlap_triangles(dt, k)
        for shape in ((70, 3), (70, 3, 2), (630,)):
            with pytest.raises(ValueError):
                r.overlap_triangles(torch.zeros(shape, device="cuda"), 4)
        with pytest.raises(ValueError):
            r.overlap_triangles(dt.double(), 4)
        with pytest.raises(TypeError):
            r.overlap_triangles_device(dt.data_ptr(), dt.data_ptr() + 12, dt.data_ptr() + 24, 70, 4, d_normal=dt.data_ptr())


def test_overlap_mesh_is_overlap_triangles_on_the_gathered_corners(soup0):
    """A mesh of 40 vertices and 90 faces about the soup: without a transform the answer is that of the gathered
    corners, and the host's; with one, that of the corners torch computes (vertices @ R.T + t in float32), read
    back and given to the host as they are."""
    import torch
    import mobileraytracer_amd as m
    rng = np.random.default_rng(131)
    verts = rng.uniform(-0.2, 1.2, (40, 3)).astype(f32)
    faces = rng.integers(0, 40, (90, 3))
    faces[::9, 2] = faces[::9, 1]  # (some segments)
    ang = 0.3
    mat = np.array([[np.cos(ang), -np.sin(ang), 0, 0.25], [np.sin(ang), np.cos(ang), 0, -0.125], [0, 0, 1, 0.5], [0, 0, 0, 1]], f32)
    dv, df = dev(verts), torch.as_tensor(faces, device="cuda")
    with m.Renderer(soup0["cfg"]) as r:
        plain = {f: x.cpu().numpy() for f, x in r.overlap_mesh(dv, df, 4).items()}
        moved_v = dv @ dev(mat)[:3, :3].T + dev(mat)[:3, 3]
        moved = {f: x.cpu().numpy() for f, x in r.overlap_mesh(dv, df, 4, transform=dev(mat)).items()}
        listed = {f: x.cpu().numpy() for f, x in r.overlap_mesh(dv, df.to(torch.int32), 4, transform=mat.tolist(), fields=("count",)).items()}
        direct = query(r, moved_v[df].reshape(-1, 9).cpu().numpy(), 4)
        empty = r.overlap_mesh(dv, df[:0], 4)
        assert empty["kind"].shape == (0, 4)
        for bad_v, bad_f in ((dv[:, :2], df), (dv, df[:, :2]), (dv, df.float()), (dv.double(), df)):
            with pytest.raises(ValueError):
                r.overlap_mesh(bad_v, bad_f, 4)
        with pytest.raises(ValueError):
            r.overlap_mesh(dv, df, 4, transform=np.eye(3, dtype=f32))
    T.assert_same(plain, soup0["lists"].expected(verts[faces].reshape(-1, 9), 4), "the mesh as it is")
    assert plain["count"].max() > 0
    T.assert_same(moved, direct, "the moved mesh against overlap_triangles on torch's corners")
    T.assert_same(moved, soup0["lists"].expected(moved_v[df].reshape(-1, 9).cpu().numpy(), 4), "the moved mesh against the host")
    assert set(listed) == {"count"} and np.array_equal(listed["count"], moved["count"])
    assert not np.array_equal(moved["count"], plain["count"])
