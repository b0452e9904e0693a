"""Extreme materials end to end: the glassboxes fixture with one coefficient made infinite, huge or
negative (tests/extreme_scenes.py), 64 x 64, depth 4, bit-exact against the oracle.

What these scenes reach that the fixture scenes do not:
* radiance outside [0, 2^32 / 255): the float -> uint32 conversion of incrementalAvg wraps negative
  values and gives 0 for NaN, +-inf and huge values (x86TruncU32);
* a non-finite Kd / Ks / Kt: ``matsFinite`` turns off the skip of the depth-capped last level, since
  Kd * 0 is then NaN and the capped children may not count as absent.

The CPU half shows on the oracle alone that every scene reaches the edge it is there for, so the GPU
half cannot pass vacuously.
"""
import functools
import os

import numpy as np
import pytest

import extreme_scenes as X

WHITTED, PATH_TRACER = 1, 2
SIZE, DEPTH = 64, 4
SENTINEL = np.int32(0x12345678)  # alpha 0x12: never produced by incrementalAvg (alpha 0xFF)
THREADS = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("extreme")
    return {name: X.write_extreme(str(d / name), name) for name in X.EXTREME}


@pytest.fixture(scope="module")
def oracle_frames(oracle_mod, scene_files):
    """(scene, shader, spp) -> (bitmap, casted rays, material count) of the oracle; rendered once."""
    @functools.lru_cache(maxsize=None)
    def get(name, shader, spp):
        obj, mtl, cam = scene_files[name]
        o = oracle_mod.Oracle(SIZE, SIZE, shader, -1, spp, 1, DEPTH, obj=obj, mtl=mtl, cam=cam)
        bm, rays = o.render(threads=THREADS)
        mats = o.counts()["materials"]
        o.close()
        bm.setflags(write=False)
        return bm, rays, mats
    return get


def red(bm):
    return bm.view(np.uint32) & 0xFF


# ---- CPU half: the oracle alone ---------------------------------------------------------------------
@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
@pytest.mark.parametrize("name", ["kd_inf", "kd_huge"])
def test_oracle_infinite_radiance_converts_to_zero(oracle_frames, name, shader):
    """Kd.r = inf, or 3e38 overflowing in flight: red is +inf or NaN in every pixel, which converts
    to 0 (a saturating conversion gives 255 for +inf)."""
    bm, _, _ = oracle_frames(name, shader, 2)
    assert (red(bm) == 0).all()  # measured: 100 % of the pixels, both scenes, both shaders


def test_oracle_negative_radiance_wraps(oracle_frames):
    bm, _, _ = oracle_frames("kd_neg", PATH_TRACER, 2)
    assert (red(bm) == 255).mean() >= 0.07  # measured: 14.9 % of the pixels (a saturating conversion: 0)


def test_oracle_nan_emission_is_no_light(oracle_frames):
    """Ke 1e39 normalises to inf / inf = NaN, which is not positive: the light's triangles become
    ordinary ones, no shadow rays are cast, and the path tracer finds no light at all."""
    for shader, want, plain in ((WHITTED, 235900, 349754), (PATH_TRACER, 605442, 840540)):  # measured
        bm, rays, _ = oracle_frames("ke_inf", shader, 2)
        assert oracle_frames("plain", shader, 2)[1] == plain
        assert rays == want and rays < plain
    assert (oracle_frames("ke_inf", PATH_TRACER, 2)[0].view(np.uint32) == 0xFF000000).all()


@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
def test_oracle_every_scene_differs_from_its_twin(oracle_frames, shader):
    plain = oracle_frames("plain", shader, 2)[0]
    for name in X.EXTREME:
        if name != "plain":
            # measured: Whitted 97.8 % (kd_neg), 99.98 % (ke_neg), 100 % (the others);
            # PathTracer 99.4 % (kd_neg), 98.3 % (ke_neg), 100 % (the others)
            assert (oracle_frames(name, shader, 2)[0] != plain).mean() >= 0.5, name


# ---- GPU half ---------------------------------------------------------------------------------------
def config(files, shader, spp, progressive=0):
    import mobileraytracer_amd as m
    obj, mtl, cam = files
    return m.Config(width=SIZE, height=SIZE, shader=shader, samplesPixel=spp, samplesLight=1, maxDepth=DEPTH,
                    sceneIndex=-1, objFilePath=obj, mtlFilePath=mtl, camFilePath=cam, progressive=progressive)


def frame(r):
    """One frame: (bitmap, rays cast by it, frame statistics)."""
    bm = np.full(SIZE * SIZE, SENTINEL, np.int32)
    before = r.get_total_casted_rays()
    r.render_frame(bm)
    return bm, r.get_total_casted_rays() - before, r.frame_stats()


def check_scene(scene_files, oracle_frames, name, shader, spp):
    import mobileraytracer_amd as m
    ref, ref_rays, ref_mats = oracle_frames(name, shader, spp)
    with m.Renderer(config(scene_files[name], shader, spp)) as r:
        assert r.scene_info()["materials"] == ref_mats
        bm, rays, st = frame(r)
        diff = int((bm != ref).sum())
        print("%s shader %d spp %d: %d of %d pixels differ, rays %d (oracle %d), walked %d of %d" % (
            name, shader, spp, diff, bm.size, rays, ref_rays, st["walkedRays"], st["rays"]))
        assert diff == 0 and rays == ref_rays
        # the flag decision (tuning key 7 = 1, the default): a non-finite Kd / Ks / Kt keeps the
        # depth-capped level's walk, shading and resolve; every other scene skips them
        assert r.get_tuning(7) == 1 and st["levelRays"][DEPTH] > 0
        if name in X.NON_FINITE:
            assert st["walkedRays"] == st["rays"]
        elif name in ("plain", "kd_huge", "kd_neg"):
            assert st["walkedRays"] == st["rays"] - st["levelRays"][DEPTH] < st["rays"]
        for key in (7, 34, 17):
            for value in (1, 0):
                r.set_tuning(key, value)
                bm, rays, _ = frame(r)
                assert np.array_equal(bm, ref) and rays == ref_rays, (name, shader, key, value)
            r.set_tuning(key, 1 if key != 17 else -1)  # back to the default
    with m.Renderer(config(scene_files[name], shader, spp, progressive=1)) as r:
        bm, rays, _ = frame(r)
        assert np.array_equal(bm, ref) and rays == ref_rays, (name, shader, "progressive")


@pytest.mark.gpu
@pytest.mark.parametrize("shader", [WHITTED, PATH_TRACER])
@pytest.mark.parametrize("name", list(X.EXTREME))
def test_extreme_scene_is_bit_equal_to_the_oracle(scene_files, oracle_frames, name, shader):
    check_scene(scene_files, oracle_frames, name, shader, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(X.EXTREME))
def test_extreme_scene_at_three_samples(scene_files, oracle_frames, name):
    """spp 3 does not divide 64: the fused resolve + accumulation is refused and k_accumulate runs."""
    check_scene(scene_files, oracle_frames, name, PATH_TRACER, 3)
