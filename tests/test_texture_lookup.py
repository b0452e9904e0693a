"""The texture lookup (Texture::loadColor, Texture.cpp:37-48; Shader::rayTrace's Kd write,
Shader.cpp:112-120) at its edges: several textures in the shared texel array, 1 / 2 / 3 / 4 channels,
16-bit samples, sizes that are no power of two, the clamp at the last texel, a map_Kd file that is
not there, two materials sharing one image, ``vt`` outside [0, 1) and the coordinates ``fract``
turns into exactly 1.0 (tests/texture_scenes.py).

* CPU half: on the palette scene every pixel's colour under DiffuseMaterial is a numpy restatement of
  loadColor on the decoded bytes of the texel its triangle names, followed by the pixel conversion of
  test_accumulate_kat.py: the oracle is pinned by a definition.
* GPU half: frames, ray counts and primary hits bit-equal to the oracle (the bars of
  test_gpu_parity.py, whose helpers are used unchanged), single frames and a batch of two views.
"""
import numpy as np
import pytest

import texture_scenes as T
from test_accumulate_kat import F, incremental_avg_np
from test_gpu_parity import coverage, gpu_hits, gpu_render, oracle_for, oracle_render

SIZE = 48
TRIANGLE = 3  # primary_hits' kind of a triangle hit


def config(paths, shader, spp=1, accelerator=3, size=SIZE, cam=None):
    import mobileraytracer_amd as m
    return m.Config(width=size, height=size, shader=shader, samplesPixel=spp, samplesLight=1, maxDepth=6,
                    sceneIndex=-1, objFilePath=paths[0], mtlFilePath=paths[1], camFilePath=cam or paths[2],
                    accelerator=accelerator)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    d = tmp_path_factory.mktemp("texture_lookup")
    pal = T.write_palette_scene(str(d / "palette"))
    cams = []
    for k in range(len(T.PALETTE_CAMS)):
        path = d / "palette" / ("view%d.cam" % k)
        path.write_text(T.palette_cam_text(k))
        cams.append(str(path))
    return {"palette": pal, "noise": T.write_noise_scene(str(d / "noise")), "palette_cams": cams}


@pytest.fixture(scope="module")
def oracle_frames(oracle_mod, scenes):
    """(scene, shader, spp, accelerator, cam) -> (bitmap, rays, primary hits) of the oracle, rendered
    once and shared, read-only."""
    cache = {}

    def get(scene, shader, spp=1, accelerator=3, cam=None):
        key = (scene, shader, spp, accelerator, cam)
        if key not in cache:
            cfg = config(scenes[scene], shader, spp, accelerator, cam=cam)
            bm, rays = oracle_render(oracle_mod, cfg)
            o = oracle_for(oracle_mod, cfg)
            hits = o.primary_hits()
            o.close()
            for a in (bm,) + tuple(hits):
                a.setflags(write=False)
            cache[key] = (bm, rays, hits)
        return cache[key]
    return get


# ---- the definition, in numpy ---------------------------------------------------------------------
def load_color_np(image, i, j):
    """Texture::loadColor at texel (i, j) of image (h, w, channels) uint8: the three bytes from the
    texel's first on (into the next texel for 1 or 2 channels), the index clamped to size - 3 where
    the reference reads past the end; each byte / 255 in float32."""
    h, w, ch = image.shape
    flat = image.reshape(-1)
    index = min(j * w * ch + i * ch, flat.size - 3 if flat.size >= 3 else 0)
    return flat[index:index + 3].astype(F) / F(255)


def palette_expected(table):
    """Per triangle of the table: the pixel DiffuseMaterial shows (Kd, then the conversion)."""
    samples = T.palette_samples()
    out = []
    for name, img, texel in table:
        if img is None:  # untextured, or the image is not there: the MTL's Kd
            kd = np.array(T.PALETTE_KD[name], F)
        else:
            depth = T.PALETTE_IMAGES[img][4]
            bytes_ = (samples[img] >> (depth - 8)).astype(np.uint8)  # 16-bit samples: the high byte
            kd = load_color_np(bytes_, *texel)
        assert (kd > 0).any()  # hasPositiveValue(Kd): DiffuseMaterial shows Kd
        out.append(incremental_avg_np(kd, np.int32(0), 1))
    return np.array(out, np.int32)


def test_palette_table_covers_the_edges():
    """The chosen texels: every corner and the last texel of every image, a last-row texel of the 1-
    and 2-channel images (their reads run into the next texel or the clamp)."""
    for name, (_, w, h, ch, _) in T.PALETTE_IMAGES.items():
        texels = set(T.PALETTE_TEXELS[name])
        assert {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)} <= texels, name
        if ch < 3:
            assert any(j == h - 1 and i < w - 1 for i, j in texels), name
    # odd sizes: every later texture starts at an odd or unaligned byte of the shared array
    sizes = [w * h * ch for _, w, h, ch, _ in T.PALETTE_IMAGES.values()]
    assert all(sum(sizes[:k]) % 4 != 0 for k in range(1, len(sizes)))


def test_oracle_palette_matches_the_definition(oracle_frames, scenes):
    table = scenes["palette"][3]
    bm, _, (kind, index, _) = oracle_frames("palette", 4)
    want = palette_expected(table)
    hit = kind == TRIANGLE
    assert hit.sum() > 0 and index[hit].max() < len(table)
    # non-vacuity: every (texture, texel) of the table is seen
    seen = np.bincount(index[hit], minlength=len(table))
    print("pixels per triangle", seen.tolist())
    assert (seen >= 4).all(), seen
    assert len({(img, texel) for _, img, texel in table if img is not None}) >= 20
    got = bm[hit]
    bad = np.nonzero(got != want[index[hit]])[0]
    assert bad.size == 0, [(table[index[hit][k]], hex(got[k] & 0xFFFFFFFF), hex(want[index[hit][k]] & 0xFFFFFFFF))
                           for k in bad[:8]]
    # two materials, one image: the same texel colours through m3 and m8
    by = {(name, texel): want[k] for k, (name, _, texel) in enumerate(table)}
    assert by[("m3", (0, 0))] == by[("m8", (0, 0))] and by[("m3", (6, 0))] == by[("m8", (6, 0))]


def test_oracle_noise_scene_is_what_it_claims(oracle_frames, scenes):
    """Neighbouring pixels of the noise quads see different texels, and the edge quads land on
    tx == 1 (the loader's fract of -1e-8)."""
    assert np.float32(-1e-8) - np.floor(np.float32(-1e-8)) == np.float32(1.0)
    quads = scenes["noise"][3]
    bm, _, (kind, index, _) = oracle_frames("noise", 4)
    on = (kind == TRIANGLE) & np.isin(index, quads["wrap"] + quads["plain"])
    distinct = len(np.unique(bm[on]))
    print("noise quads: pixels", int(on.sum()), "distinct colours", distinct)
    assert on.sum() >= 600 and 2 * distinct >= on.sum()
    for name in ("edge_u", "edge_uv"):
        assert ((kind == TRIANGLE) & np.isin(index, quads[name])).sum() >= 100, name


# ---- GPU --------------------------------------------------------------------------------------------
CASES = [  # shader, spp, accelerator
    (4, 1, 3), (0, 1, 3), (1, 1, 3), (2, 4, 3), (1, 1, 1), (1, 1, 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["palette", "noise"])
@pytest.mark.parametrize("case", CASES, ids=["sh%d-spp%d-acc%d" % c for c in CASES])
def test_frames_bit_equal_to_the_oracle(oracle_frames, scenes, scene, case):
    shader, spp, accelerator = case
    ref, ref_rays, ref_hits = oracle_frames(scene, shader, spp, accelerator)
    if scene == "noise":  # non-vacuity, on the oracle's frame before any comparison
        quads = scenes["noise"][3]
        d = oracle_frames("noise", 4)
        on = (d[2][0] == TRIANGLE) & np.isin(d[2][1], quads["wrap"] + quads["plain"])
        assert 2 * len(np.unique(d[0][on])) >= on.sum() >= 600
    cfg = config(scenes[scene], shader, spp, accelerator)
    bm, rays, _ = gpu_render(cfg)
    once = coverage(cfg.width, cfg.height) == 1
    diff = int((bm[once] != ref[once]).sum())
    print(scene, case, "differing pixels", diff, "rays", rays, ref_rays)
    assert diff == 0
    assert rays == ref_rays
    assert len(np.unique(bm)) > 1
    k, i, t = gpu_hits(cfg)
    assert np.array_equal(k, ref_hits[0]) and np.array_equal(i, ref_hits[1])
    assert np.array_equal(t.view(np.int32), ref_hits[2].view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("shader,spp", [(4, 1), (1, 1), (2, 4)])
def test_palette_views_bit_equal_to_the_oracle(oracle_frames, scenes, shader, spp):
    """A batch of two views (the batched kernels are instantiations of their own): each view equals
    the oracle's frame for that camera."""
    import mobileraytracer_amd as m
    cams = scenes["palette_cams"]
    refs = [oracle_frames("palette", shader, spp, 3, cam) for cam in cams]
    assert not np.array_equal(refs[0][0], refs[1][0])
    with m.Renderer(config(scenes["palette"], shader, spp)) as r:
        bms = np.full((len(cams), SIZE * SIZE), 0x12345678, np.int32)
        r.render_views(T.palette_views(), bms)
        rays = r.get_total_casted_rays()
    for v, ref in enumerate(refs):
        diff = int((bms[v] != ref[0]).sum())
        print("view", v, "differing pixels", diff)
        assert diff == 0, "view %d differs from the oracle" % v
    assert rays == sum(ref[1] for ref in refs)
