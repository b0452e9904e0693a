"""Dispatch boundaries that the scene's content and the sample count decide.

* The lean k_shade copies the materials and lights into a 256-entry float4 LDS table (4 records per
  material, then 4 per light) and the launch takes the general kernel when they do not fit
  (launchShade).  tests/extreme_scenes.py generates scenes one record under, at and over that limit,
  far over it, and one with many lights (lightChoice, the lights' offset behind the materials).
  Every material has its own exactly representable Kd, so a record read from the wrong table slot
  changes the image.
* launchResolveAccumulate folds level 1's resolve into the accumulation when spp divides 64 (a
  slot's samples then share a wave) and is refused otherwise: every other divisor up to a slot that
  fills a whole wave, the refusals, and a last wave partly past the frame's paths.

Everything is bit-exact against the oracle.
"""
import functools
import os

import numpy as np
import pytest

import extreme_scenes as X

WHITTED, PATH_TRACER = 1, 2
SENTINEL = np.int32(0x12345678)  # alpha 0x12: never produced by incrementalAvg (alpha 0xFF)
THREADS = min(16, os.cpu_count() or 1)
LDS_TABLE = 256  # kShadeLdsTable (mrt_kernels.hip)

# ---- 1. table sizes -----------------------------------------------------------------------------------
SIZE, DEPTH, SPP = 64, 3, 2
# name -> (grid materials M, emissive quads Q, lean kernel expected): M + 2 materials, 2 Q lights
TABLE_CASES = {
    "one_under": (57, 2, True),     # 59 + 4 = 63 records of 4 float4
    "at_limit": (58, 2, True),      # 64: the table is full
    "one_over": (59, 2, False),     # 65: the general kernel
    "far_over": (300, 2, False),    # 306
    "many_lights": (20, 20, True),  # 22 + 40 = 62: the lights' half of the table is the larger
}


@pytest.fixture(scope="module")
def table_scenes(tmp_path_factory):
    d = tmp_path_factory.mktemp("tables")
    return {name: X.write_table_scene(str(d / name), m, q) for name, (m, q, _) in TABLE_CASES.items()}


@pytest.fixture(scope="module")
def table_oracle(oracle_mod, table_scenes):
    @functools.lru_cache(maxsize=None)
    def get(name, shader):
        obj, mtl, cam = table_scenes[name]
        o = oracle_mod.Oracle(SIZE, SIZE, shader, -1, SPP, 1, DEPTH, obj=obj, mtl=mtl, cam=cam)
        bm, rays = o.render(threads=THREADS)
        counts = o.counts()
        o.close()
        bm.setflags(write=False)
        return bm, rays, counts
    return get


def frame(r, n):
    bm = np.full(n, SENTINEL, np.int32)
    before = r.get_total_casted_rays()
    r.render_frame(bm)
    st = r.frame_stats()
    return bm, r.get_total_casted_rays() - before, (st["rays"], st["shadowRays"], tuple(st["levelRays"]))


@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_table_scenes_on_the_oracle(table_oracle, name, shader):
    """No GPU: the generated scenes have the materials and lights they are meant to, and an image of
    many colours."""
    n_mats, n_quads, _ = TABLE_CASES[name]
    ref, _, counts = table_oracle(name, shader)
    assert (counts["materials"], counts["lights"]) == (n_mats + 2, 2 * n_quads)
    assert len(np.unique(ref)) > 1000  # measured: 1280 - 2689 distinct pixel values


@pytest.mark.gpu
@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_table_size_boundary(table_scenes, table_oracle, name, shader):
    import mobileraytracer_amd as m
    n_mats, n_quads, lean = TABLE_CASES[name]
    obj, mtl, cam = table_scenes[name]
    ref, ref_rays, _ = table_oracle(name, shader)
    cfg = m.Config(width=SIZE, height=SIZE, shader=shader, samplesPixel=SPP, samplesLight=1, maxDepth=DEPTH,
                   sceneIndex=-1, objFilePath=obj, mtlFilePath=mtl, camFilePath=cam)
    with m.Renderer(cfg) as r:
        info = r.scene_info()
        assert (info["materials"], info["lights"]) == (n_mats + 2, 2 * n_quads)
        # the table the lean kernel would need, as launchShade counts it
        assert (X.table_records(info["materials"], info["lights"]) <= LDS_TABLE) == lean
        first = None
        for key in (10, 17):
            for value in (1, 0):
                r.set_tuning(key, value)
                bm, rays, stats = frame(r, SIZE * SIZE)
                assert np.array_equal(bm, ref) and rays == ref_rays, (name, shader, key, value)
                first = first or stats
                assert stats == first, (name, shader, key, value)
            r.set_tuning(key, 1 if key == 10 else -1)  # back to the default


def test_table_cases_straddle_the_limit():
    sizes = {name: X.table_records(m + 2, 2 * q) for name, (m, q, _) in TABLE_CASES.items()}
    assert sizes["one_under"] == LDS_TABLE - 4 and sizes["at_limit"] == LDS_TABLE
    assert sizes["one_over"] == LDS_TABLE + 4 and sizes["far_over"] > 4 * LDS_TABLE
    assert sizes["many_lights"] <= LDS_TABLE and TABLE_CASES["many_lights"][1] * 2 == 40


# ---- 2. sample counts ---------------------------------------------------------------------------------
CW, CDEPTH = 32, 3
SPPS = [5, 6, 7, 16, 32, 64, 128]  # 64 % spp == 0: fused (16, 32, 64: a slot fills a whole wave); else refused
UP = (0.0, 1.0, 0.0)
VIEWS = [(0, (0.4, 0.2, -3.0), (0.0, 0.0, 1.0), UP, 50.0, 40.0),
         (0, (-0.6, 0.3, -2.6), (0.1, -0.1, 1.0), UP, 60.0, 45.0)]


@pytest.fixture(scope="module")
def cornell_oracle(oracle_mod):
    @functools.lru_cache(maxsize=None)
    def get(spp):
        bm, rays = oracle_mod.Oracle(CW, CW, PATH_TRACER, 0, spp, 1, CDEPTH).render(threads=THREADS)
        bm.setflags(write=False)
        return bm, rays
    return get


def cornell(spp, progressive=0):
    import mobileraytracer_amd as m
    return m.Config(width=CW, height=CW, shader=PATH_TRACER, sceneIndex=0, samplesPixel=spp, maxDepth=CDEPTH,
                    progressive=progressive)


@pytest.mark.gpu
@pytest.mark.parametrize("spp", SPPS)
def test_sample_count_boundary(cornell_oracle, spp):
    import mobileraytracer_amd as m
    ref, ref_rays = cornell_oracle(spp)
    for progressive in (0, 1):
        with m.Renderer(cornell(spp, progressive)) as r:
            for fused in (1, 0):
                r.set_tuning(34, fused)
                bm, rays, _ = frame(r, CW * CW)
                assert np.array_equal(bm, ref) and rays == ref_rays, (spp, progressive, fused)
            assert r.get_sample() == spp


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [s for s in SPPS if s >= 16])
def test_sample_count_in_a_batch_of_views(spp):
    """The kViews instantiations of the same kernels: a 2-view batch against the set_camera loop."""
    import mobileraytracer_amd as m
    with m.Renderer(cornell(spp)) as r:
        singles, rays = np.full((2, CW * CW), SENTINEL, np.int32), 0
        for v, cam in enumerate(VIEWS):
            r.set_camera(*cam)
            bm, n, _ = frame(r, CW * CW)
            singles[v] = bm
            rays += n
        assert not (singles == SENTINEL).any() and not np.array_equal(singles[0], singles[1])
        for fused in (1, 0):
            r.set_tuning(34, fused)
            bms = np.full((2, CW * CW), SENTINEL, np.int32)
            before = r.get_total_casted_rays()
            r.render_views(VIEWS, bms)
            assert np.array_equal(bms, singles), (spp, fused)
            assert r.get_total_casted_rays() - before == rays
