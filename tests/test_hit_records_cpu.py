"""Surface records without a device: the host-only scene accessors (mrt_scene_triangles / _planes /
_spheres / _materials / _lights) against the oracle's counts, the triangle BVH and the generated room's
own description, and the argument errors of mrt_cast_hits_device that are checked before the renderer
is read.

Float comparisons are exact: the expected values are computed in float32, one operation at a time, in
mrt_common.hpp's order: dot = (x x' + y y') + z z', normalize = v * (1 / sqrt(dot(v, v)))."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hit_scenes as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_BYTES = 1 << 16
FILL = b"\xa5"
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(x, y):  # glm::cross
    return np.stack([x[..., 1] * y[..., 2] - y[..., 1] * x[..., 2], x[..., 2] * y[..., 0] - y[..., 2] * x[..., 0],
                     x[..., 0] * y[..., 1] - y[..., 0] * x[..., 1]], -1)


def normalize(v):
    v = np.asarray(v, np.float32)
    return v * (f32(1.0) / np.sqrt(dot(v, v)))[..., None]


def ulps(a, b):
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    return H.write_room(str(tmp_path_factory.mktemp("hit_room")))


def room_cfg(room, **kw):
    import mobileraytracer_amd as m
    return m.Config(width=16, height=16, shader=1, sceneIndex=-1, objFilePath=room[0], mtlFilePath=room[1],
                    camFilePath=room[2], **kw)


def water_cfg():
    import mobileraytracer_amd as m
    from mobileraytracer_amd import scenes
    obj, mtl, cam = scenes.cornell_water()
    return m.Config(width=16, height=16, shader=1, sceneIndex=-1, objFilePath=obj, mtlFilePath=mtl, camFilePath=cam)


def all_cfgs(room):
    import mobileraytracer_amd as m
    return {"water": water_cfg(), "scene2": m.Config(width=16, height=16, sceneIndex=2),
            "scene3": m.Config(width=16, height=16, sceneIndex=3), "room": room_cfg(room)}


def oracle_of(oracle_mod, cfg):
    return oracle_mod.Oracle(cfg.width, cfg.height, cfg.shader, cfg.sceneIndex, cfg.samplesPixel, cfg.samplesLight,
                             cfg.maxDepth, obj=cfg.objFilePath, mtl=cfg.mtlFilePath, cam=cfg.camFilePath,
                             accelerator=cfg.accelerator)


# ---- the accessors -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["water", "scene2", "scene3", "room"])
def test_accessor_counts_equal_the_oracles(oracle_mod, native_lib_path, room, name):
    import mobileraytracer_amd as m
    cfg = all_cfgs(room)[name]
    ob = oracle_of(oracle_mod, cfg)
    want = ob.counts()
    ob.close()
    geom, normals, tex, tmat = m.scene_triangles(cfg)
    planes, pmat = m.scene_planes(cfg)
    spheres, smat = m.scene_spheres(cfg)
    coeffs, texture = m.scene_materials(cfg)
    lkind, lgeom, lcoeffs = m.scene_lights(cfg)
    got = dict(triangles=len(geom), lights=len(lkind), planes=len(planes), spheres=len(spheres), materials=len(coeffs))
    assert got == {k: want[k] for k in got}
    assert geom.shape == (got["triangles"], 3, 3) and normals.shape == geom.shape and tex.shape == (len(geom), 3, 2)
    assert planes.shape == (got["planes"], 2, 3) and spheres.shape == (got["spheres"], 4)
    assert coeffs.shape == (got["materials"], 13) and lgeom.shape == (got["lights"], 3, 3) and lcoeffs.shape == (len(lkind), 13)
    # every material index names a material
    for mat in (tmat, pmat, smat):
        assert mat.dtype == np.int32 and ((mat >= 0) & (mat < got["materials"])).all()
    assert ((texture >= -1)).all()
    if name == "room":
        assert got["triangles"] == 50 and got["lights"] == 2 and got["triangles"] == len(room[3])


@pytest.mark.parametrize("name", ["water", "scene2", "room"])
def test_triangle_corners_lie_in_the_bvh_root_box(native_lib_path, room, name):
    import mobileraytracer_amd as m
    cfg = all_cfgs(room)[name]
    geom = m.scene_triangles(cfg)[0]
    boxes, _, _, order = m.triangle_bvh(cfg)
    lo, hi = boxes[0, :3], boxes[0, 3:]
    a = geom[:, 0]
    corners = np.stack([a, a + geom[:, 1], a + geom[:, 2]], 1)
    assert (corners >= lo).all() and (corners <= hi).all()
    # ... and touch it: the box is the union of exactly these triangles
    assert np.array_equal(corners.reshape(-1, 3).min(0), lo) and np.array_equal(corners.reshape(-1, 3).max(0), hi)
    assert sorted(order.tolist()) == list(range(len(geom)))


def test_flat_normals_are_the_loaders_face_normal(native_lib_path, room):
    """A face without ``vn``: the loader takes normalize(cross(AC, AB)) (OBJLoader.cpp:176-182) and
    Triangle's constructor normalises its normals again (Triangle.cpp:18-20), so the stored normal is
    that expression normalised twice - from the accessor's own AB and AC, bit for bit."""
    import mobileraytracer_amd as m
    geom, normals, _, _ = m.scene_triangles(room_cfg(room))
    flat = np.array([not t["smooth"] for t in room[3]])
    assert flat.sum() >= 16 + 2 and (~flat).sum() >= 16
    want = normalize(normalize(cross(geom[flat, 2], geom[flat, 1])))
    for k in range(3):
        assert np.array_equal(bits(normals[flat, k]), bits(want))
    # the two corner panels: no axis, so the normalisation is not trivial
    assert (np.abs(want).max(1) < 0.99).sum() == 2
    # the built-in scenes' triangles (Triangle::Builder, Triangle.cpp:328-339) have the same face normal
    g2, n2, _, _ = m.scene_triangles(m.Config(sceneIndex=2))
    w2 = normalize(normalize(cross(g2[:, 2], g2[:, 1])))
    for k in range(3):
        assert len(g2) == 2 and np.array_equal(bits(n2[:, k]), bits(w2))


def test_smooth_normals_are_the_files_normals_normalised(native_lib_path, room):
    """A face with ``vn``: (-x, y, z) of the file's normal (OBJLoader.cpp:170-172), normalised once by
    Triangle's constructor."""
    import mobileraytracer_amd as m
    _, normals, _, _ = m.scene_triangles(room_cfg(room))
    checked = 0
    for k, t in enumerate(room[3]):
        if not t["smooth"]:
            continue
        pre = np.array(t["vn"], np.float32) * np.array([-1.0, 1.0, 1.0], np.float32)
        assert np.array_equal(bits(normals[k]), bits(normalize(pre)))
        assert (ulps(dot(normals[k], normals[k]), np.ones(3, np.float32)) <= 2).all()
        assert not (np.array_equal(normals[k, 0], normals[k, 1]) and np.array_equal(normals[k, 0], normals[k, 2]))
        checked += 1
    assert checked == 24


def test_room_materials_are_what_the_generator_wrote(native_lib_path, room):
    import mobileraytracer_amd as m
    cfg = room_cfg(room)
    _, _, tex, tmat = m.scene_triangles(cfg)
    coeffs, texture = m.scene_materials(cfg)
    lkind, lgeom, lcoeffs = m.scene_lights(cfg)
    names = {}
    for k, t in enumerate(room[3]):
        assert names.setdefault(int(tmat[k]), t["material"]) == t["material"]  # one index per MTL material
        # texture coordinates exactly where the material has an image, inside [0, 1)
        if t["textured"]:
            assert (tex[k] >= 0).all() and (tex[k] < 1).all()
        else:
            assert (tex[k] == -1).all()
    assert sorted(names) == list(range(len(coeffs))) and set(names.values()) == {"plain", "blue", "tex", "gloss"}

    def row(d):
        return np.array(d["le"] + d["kd"] + d["ks"] + d["kt"] + (d["ior"],), np.float32)

    for index, name in names.items():
        assert np.array_equal(bits(coeffs[index]), bits(row(H.MATERIALS[name]))), name
        assert (texture[index] == -1) == (H.MATERIALS[name]["image"] is None)
    assert sorted(texture[texture >= 0].tolist()) == [0]
    # the emissive quad: two area lights with the normalised Ke
    assert lkind.tolist() == [1, 1]
    for k in range(2):
        assert np.array_equal(bits(lcoeffs[k]), bits(row(H.MATERIALS["light"])))
        assert (lgeom[k, 0, 1] == f32(H.Y1 - 1.0 / 64.0))


def test_builtin_planes_and_spheres(native_lib_path):
    """Scene 3 (Scenes.cpp:264-302): a floor plane through the origin and five spheres; scene 2: six
    planes with unit normals."""
    import mobileraytracer_amd as m
    planes, pmat = m.scene_planes(m.Config(sceneIndex=3))
    spheres, smat = m.scene_spheres(m.Config(sceneIndex=3))
    assert planes.tolist() == [[[0.0, 1.0, 0.0], [0.0, 0.0, 0.0]]] and len(spheres) == 5
    assert (spheres[:, 3] > 0).all() and len(set(smat.tolist()) | set(pmat.tolist())) == len(m.scene_materials(m.Config(sceneIndex=3))[0])
    planes2, _ = m.scene_planes(m.Config(sceneIndex=2))
    assert len(planes2) == 6 and np.array_equal(dot(planes2[:, 0], planes2[:, 0]), np.ones(6, np.float32))
    lkind, lgeom, lcoeffs = m.scene_lights(m.Config(sceneIndex=2))
    assert lkind.tolist() == [1, 1] and (lcoeffs[:, 0:3] > 0).all()
    lkind3, lgeom3, _ = m.scene_lights(m.Config(sceneIndex=3))
    assert lkind3.tolist() == [0] and lgeom3[0].tolist() == [[0.0, 15.0, 4.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]


def test_accessors_report_a_scene_that_cannot_be_loaded(native_lib_path):
    import mobileraytracer_amd as m
    with pytest.raises(RuntimeError, match="cannot open OBJ"):
        m.scene_triangles(m.Config(sceneIndex=-1, objFilePath="/nonexistent/none.obj"))


# ---- argument errors of mrt_cast_hits_device -----------------------------------------------------------
@pytest.fixture(scope="module")
def lib(native_lib_path):
    from mobileraytracer_amd import _native
    return _native.load_library(native_lib_path)


@pytest.fixture()
def fake():
    """An opaque block standing in for the renderer: the batch and the outputs are checked before the
    renderer is read, so it is never dereferenced (and never written: checked after each call)."""
    block = ctypes.create_string_buffer(FILL * FAKE_BYTES, FAKE_BYTES)
    yield block
    assert block.raw == FILL * FAKE_BYTES


def _batch(**kw):
    from mobileraytracer_amd import _native
    f = dict(orig=0x1000, dir=0x2000, dist=None, src=None, origStride=3, dirStride=3, n=4)
    f.update(kw)
    return _native.MrtRayBatch(**f)


def _records(**kw):
    """All thirteen fields set (the pointers stand for device memory: never dereferenced here)."""
    from mobileraytracer_amd import _native
    f = {name: 0x10000 * (k + 1) for k, (name, _, _) in enumerate(_native.HIT_FIELDS)}
    f.update(kw)
    return _native.MrtHitRecords(**f)


def _call(lib, handle, batch, rec, size=None):
    size = ctypes.sizeof(rec) if size is None and rec is not None else (size or 0)
    rc = lib.mrt_cast_hits_device(handle, None if batch is None else ctypes.byref(batch),
                                  None if rec is None else ctypes.byref(rec), size, None)
    return rc, lib.mrt_last_error()


def test_cast_hits_rejects_null_arguments(lib, fake):
    rc, msg = _call(lib, None, _batch(), _records())
    assert rc == -1 and b"mrt_cast_hits_device" in msg and b"null renderer" in msg
    rc, msg = _call(lib, fake, None, _records())
    assert rc == -1 and b"null ray batch" in msg
    rc, msg = _call(lib, fake, _batch(), None, 104)
    assert rc == -1 and b"null hit records" in msg
    for field in ("orig", "dir"):
        rc, msg = _call(lib, fake, _batch(**{field: None}), _records())
        assert rc == -1 and b"null" in msg and field.encode() in msg


@pytest.mark.parametrize("size", [0, 1, 7])
def test_cast_hits_rejects_a_size_that_cannot_hold_kind(lib, fake, size):
    rec = _records()
    rc = lib.mrt_cast_hits_device(fake, ctypes.byref(_batch()), ctypes.byref(rec), size, None)
    assert rc == -1 and b"outSize" in lib.mrt_last_error()


def test_cast_hits_rejects_no_wanted_output(lib, fake):
    from mobileraytracer_amd import _native
    none = {name: None for name, _, _ in _native.HIT_FIELDS}
    rc, msg = _call(lib, fake, _batch(), _records(**none))
    assert rc == -1 and b"no output" in msg
    # fields beyond outSize count as null: only kind, index, t are within 24 bytes
    rec = _records(kind=None, index=None, t=None)
    rc, msg = _call(lib, fake, _batch(), rec, 24)
    assert rc == -1 and b"no output" in msg
    # ... and a field cut in half is not within it
    rec = _records(kind=None, index=None, t=None)
    rc, msg = _call(lib, fake, _batch(), rec, 31)
    assert rc == -1 and b"no output" in msg


@pytest.mark.parametrize("n", [0, -1, 1 << 31, -(1 << 31), 1 << 40])
def test_cast_hits_rejects_a_count_outside_the_int_range(lib, fake, n):
    rc, msg = _call(lib, fake, _batch(n=n), _records())
    assert rc == -1 and b"n must be" in msg


@pytest.mark.parametrize("field", ["origStride", "dirStride"])
@pytest.mark.parametrize("stride", [1, 2, -1, -(1 << 40)])
def test_cast_hits_rejects_a_stride_below_three(lib, fake, field, stride):
    rc, msg = _call(lib, fake, _batch(**{field: stride}), _records())
    assert rc == -1 and field.encode() in msg


def test_hit_records_struct_matches_the_header(tmp_path):
    """ctypes MrtHitRecords has the size and the field offsets of the C mrt_hit_records, and the new
    symbols are exported."""
    from mobileraytracer_amd import _native
    fields = [name for name, _, _ in _native.HIT_FIELDS]
    assert [f for f, _ in _native.MrtHitRecords._fields_] == fields
    src = tmp_path / "records.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mobilert_amd.h"\n'
                   'int main(void){printf("%zu", sizeof(mrt_hit_records));'
                   + "".join('printf(" %%zu", offsetof(mrt_hit_records, %s));' % f for f in fields) + 'return 0;}')
    exe = tmp_path / "records"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_native.MrtHitRecords)] + [getattr(_native.MrtHitRecords, f).offset for f in fields]
    assert got == [104] + [8 * k for k in range(13)]
    assert {"mrt_cast_hits_device", "mrt_scene_triangles", "mrt_scene_planes", "mrt_scene_spheres",
            "mrt_scene_materials", "mrt_scene_lights"} <= set(_native.EXPORTED_SYMBOLS)
