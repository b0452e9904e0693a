"""The shared-Kd replay (Shader.cpp:112-120: a textured hit overwrites its material's Kd, which a
shade() that traced a child first reads afterwards; DESIGN.md deviation 4) with more than one
textured material and after transmission subtrees.

The scene is a corridor of two facing mirrors, floor material X and ceiling material Y, each with a
noise image of its own (tests/texture_scenes.py): a floor vertex's specular subtree is Y, X, Y, ...,
so the subtree's last write is to Y as often as to X, and the Kd the floor vertex reads after it is
the last write to X INSIDE that subtree.  With ``kt`` material X also transmits and a slab of it
stands across the corridor, so the ambient term reads Kd after a transmission subtree.

* CPU half: the case is what it claims - the sixth level reaches the image, the chain of materials
  alternates down to level 5 and the X texels at levels 1 and 5 differ.
* GPU half: frames and ray counts bit-equal to the oracle, Whitted at depths 2, 3 and 6 and the
  PathTracer at 4 spp and depth 6, in one pass and in chunked passes.

Measured once on an MI355X with the replay that kept only a subtree's last write, whatever its
material (profiles/texture_replay_bench.txt): cases (a) and (b) equal the oracle; case (c) differs in
851 of 1024 pixels under Whitted at depth 6, 847 at depth 3, 0 at depth 2, and 1016 under the
PathTracer; case (d) in 1023, 653, 124 and 1008.
"""
import functools

import numpy as np
import pytest

import texture_scenes as T
from test_gpu_parity import gpu_render, oracle_render

SIZE = 32
WHITTED, PATH_TRACER = 1, 2
TRIANGLE = 3
CASES = {  # name -> (textured, kt)
    "a": (("X",), False),       # the supported domain of the parent: deep S subtrees
    "b": (("X",), True),        # Kd read after a transmission subtree
    "c": (("X", "Y"), False),   # two textured materials
    "d": (("X", "Y"), True),
}
RUNS = [  # shader, spp, depth
    (WHITTED, 1, 6), (WHITTED, 1, 2), (WHITTED, 1, 3), (PATH_TRACER, 4, 6),
]


def config(paths, shader, spp, depth):
    import mobileraytracer_amd as m
    return m.Config(width=SIZE, height=SIZE, shader=shader, samplesPixel=spp, samplesLight=1, maxDepth=depth,
                    sceneIndex=-1, objFilePath=paths[0], mtlFilePath=paths[1], camFilePath=paths[2])


@pytest.fixture(scope="module")
def corridors(tmp_path_factory):
    d = tmp_path_factory.mktemp("texture_replay")
    return {name: T.write_corridor(str(d / name), textured, kt) for name, (textured, kt) in CASES.items()}


@pytest.fixture(scope="module")
def oracle_frames(oracle_mod, corridors):
    """(case, shader, spp, depth) -> (bitmap, rays) of the oracle, rendered once, shared, read-only."""
    @functools.lru_cache(maxsize=None)
    def get(case, shader, spp, depth):
        bm, rays = oracle_render(oracle_mod, config(corridors[case], shader, spp, depth))
        bm.setflags(write=False)
        return bm, rays
    return get


# ---- CPU: the case is what it claims ----------------------------------------------------------------
@pytest.mark.parametrize("case", ["c", "d"])
def test_sixth_level_writes_reach_the_image(oracle_frames, case):
    d6, _ = oracle_frames(case, WHITTED, 1, 6)
    d5, _ = oracle_frames(case, WHITTED, 1, 5)
    differ = int((d6 != d5).sum())
    print("case", case, "depth 6 vs depth 5:", differ, "of", d6.size, "pixels differ")
    assert 10 * differ >= d6.size
    for shader, spp in ((WHITTED, 1), (PATH_TRACER, 4)):  # a lit picture, not a few flat colours
        bm, _ = oracle_frames(case, shader, spp, 6)
        assert len(np.unique(bm)) >= d6.size // 2, (shader, len(np.unique(bm)))


def camera_rays(oracle_mod, cam):
    """The centre ray of every pixel of a SIZE x SIZE frame (Perspective.cpp:14-25), in float64."""
    c = oracle_mod.kat_camera(cam, 1.0)
    pos, direction, up, right = (np.array(c[k], np.float64) for k in ("position", "direction", "up", "right"))
    hfov, vfov = np.radians(c["hfov"]), np.radians(c["vfov"])
    ys, xs = (a.ravel() for a in np.mgrid[0:SIZE, 0:SIZE])
    rf = np.array([oracle_mod.fast_arctan(float(hfov * (x / SIZE - 0.5))) for x in xs])
    uf = np.array([oracle_mod.fast_arctan(float(vfov * (0.5 - y / SIZE))) for y in ys])
    d = direction[None] + right[None] * rf[:, None] + up[None] * uf[:, None]
    return np.repeat(pos[None], SIZE * SIZE, 0), d / np.linalg.norm(d, axis=1, keepdims=True)


def test_material_chain_alternates_to_level_five(oracle_mod, corridors):
    """For a sample of pixels: the specular chain's materials are X, Y, X, Y, X, ... (followed with the
    oracle's ray casts and a float64 reflect; only the ids matter), and the texels of X at levels 1
    and 5 differ, so a replay that hands level 1 its own texel back is visibly wrong."""
    obj, mtl, cam, tris = corridors["c"]
    o = oracle_mod.Oracle(SIZE, SIZE, WHITTED, -1, 1, 1, 6, obj=obj, mtl=mtl, cam=cam)
    orig, dirs = camera_rays(oracle_mod, cam)
    pk, pi, _ = o.primary_hits()
    material = {j: name for name in ("X", "Y") for j in tris[name]}
    sample = [y * SIZE + x for y in range(14, 32, 3) for x in range(2, 32, 3)]
    orig, dirs = orig[sample], dirs[sample]
    chains, points = [[] for _ in sample], [[] for _ in sample]
    src = None
    for level in range(1, 7):
        k, i, t = o.trace_rays(orig, dirs, src=src)
        if level == 1:  # the float64 camera model names the oracle's own primary hits
            assert np.array_equal(k, pk[sample]) and np.array_equal(i, pi[sample])
        for n in range(len(sample)):
            if len(chains[n]) == level - 1 and k[n] == TRIANGLE:
                chains[n].append(material[int(i[n])])
                points[n].append(orig[n] + float(t[n]) * dirs[n])
        orig = orig + t[:, None].astype(np.float64) * dirs
        dirs = dirs * np.array([1.0, -1.0, 1.0])  # reflect about the floor's / ceiling's normal (0, +-1, 0)
        src = np.stack([k, i], 1).astype(np.int32)
    o.close()
    different = 0
    for n, chain in enumerate(chains):
        assert len(chain) >= 5 and chain[:6] == ["X", "Y", "X", "Y", "X", "Y"][:len(chain)], (sample[n], chain)
        p1, p5 = points[n][0], points[n][4]
        # (the loader negates x: file-space x = -x)
        different += T.corridor_texel("X", -p1[0], p1[2]) != T.corridor_texel("X", -p5[0], p5[2])
    print("sample", len(sample), "pixels; X texels at levels 1 and 5 differ in", different)
    assert different == len(sample)


# ---- GPU ----------------------------------------------------------------------------------------------
def check(case, run, bm, rays, ref, ref_rays):
    diff = int((bm != ref).sum())
    worst = int(np.abs(((bm[:, None] >> np.array([0, 8, 16])) & 0xFF) - ((ref[:, None] >> np.array([0, 8, 16])) & 0xFF)).max())
    print("case", case, "run", run, "differing pixels", diff, "of", bm.size, "largest channel difference", worst)
    assert diff == 0
    assert rays == ref_rays


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS, ids=["whitted-d6", "whitted-d2", "whitted-d3", "pathtracer-spp4-d6"])
@pytest.mark.parametrize("case", list(CASES))
def test_corridor_bit_equal_to_the_oracle(oracle_frames, corridors, case, run):
    shader, spp, depth = run
    ref, ref_rays = oracle_frames(case, shader, spp, depth)
    bm, rays, _ = gpu_render(config(corridors[case], shader, spp, depth))
    check(case, run, bm, rays, ref, ref_rays)


@pytest.mark.gpu
@pytest.mark.parametrize("shader,spp,budget", [(WHITTED, 1, 2), (PATH_TRACER, 4, 4)])
@pytest.mark.parametrize("case", list(CASES))
def test_corridor_in_chunked_passes(oracle_frames, corridors, case, shader, spp, budget):
    """A queue budget of `budget` MiB with 64 slots of slack per segment (tuning keys 37 and 39; key 37
    as in test_forced_small_budget_renders_in_chunks): the first plan's chunk is 637 / 358 of the 1024
    pixel slots (plan_queues), so the frame renders in several chunks."""
    import mobileraytracer_amd as m
    ref, ref_rays = oracle_frames(case, shader, spp, 6)
    cfg = config(corridors[case], shader, spp, 6)
    with m.Renderer(cfg) as r:
        r.set_tuning(39, 64)
        r.set_tuning(37, budget)
        bm = np.full(SIZE * SIZE, 0x12345678, np.int32)
        r.render_frame(bm)
        rays = r.get_total_casted_rays()
        q = r.queue_info()
    print("chunked", q)
    assert q["chunkSlots"] < SIZE * SIZE and q["passes"] > 1
    check(case, (shader, spp, 6, "chunked"), bm, rays, ref, ref_rays)
