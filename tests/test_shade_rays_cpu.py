"""mrt_shade_rays_device / mrt_camera_rays_device / mrt_path_key without a device: the host-only path
key against the oracle's, the ctypes mirrors of the header's structs, and the argument errors that
are checked before any device work (and before the renderer is read)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_BYTES = 1 << 16
FILL = b"\xa5"


@pytest.fixture(scope="module")
def lib(native_lib_path):
    from mobileraytracer_amd import _native
    return _native.load_library(native_lib_path)


@pytest.fixture()
def fake():
    """An opaque block standing in for the renderer: the batch and the output are checked before the
    renderer is read, so it is never dereferenced (and never written: checked after each call)."""
    block = ctypes.create_string_buffer(FILL * FAKE_BYTES, FAKE_BYTES)
    yield block
    assert block.raw == FILL * FAKE_BYTES


def _batch(key=0x7000, **kw):
    """A well-formed shade batch of 4 rays (the pointers stand for device memory: never dereferenced
    on the paths tested here), with the given ray fields replaced."""
    from mobileraytracer_amd import _native
    f = dict(orig=0x1000, dir=0x2000, dist=None, src=None, origStride=3, dirStride=3, n=4)
    f.update(kw)
    return _native.MrtShadeBatch(_native.MrtRayBatch(**f), key or None)


def _call(lib, handle, batch, rgb=0x4000, rgb_stride=3):
    rays = (ctypes.c_uint64 * 2)(77, 77)
    rc = lib.mrt_shade_rays_device(handle, None if batch is None else ctypes.byref(batch), ctypes.c_void_p(rgb or None),
                                   rgb_stride, rays, None)
    assert list(rays) == [77, 77]  # nothing done
    return rc, lib.mrt_last_error()


def test_path_key_is_the_oracles(lib, oracle_mod):
    import mobileraytracer_amd as m
    rng = np.random.default_rng(20261020)
    top = (1 << 32) - 1
    pairs = [(0, 0), (0, top), (top, 0), (top, top), (1, 0), (0, 1), (255, 3), (16 * 16 - 1, 3), (1 << 31, 1 << 31)]
    pairs += [(int(p), int(s)) for p, s in zip(rng.integers(0, 1 << 32, 300), rng.integers(0, 1 << 32, 300))]
    pairs += [(int(p), int(s)) for p, s in zip(rng.integers(0, 1920 * 1080, 100), rng.integers(0, 64, 100))]
    got = [m.path_key(p, s) for p, s in pairs]
    assert got == [oracle_mod.path_key(p, s) for p, s in pairs]
    assert got == [lib.mrt_path_key(p, s) for p, s in pairs]
    assert len(set(got)) > 400  # (a key, not a constant)


def test_shade_rays_rejects_a_null_handle(lib):
    rc, msg = _call(lib, None, _batch())
    assert rc == -1 and b"mrt_shade_rays_device" in msg and b"null renderer" in msg


def test_shade_rays_rejects_a_null_batch(lib, fake):
    rc, msg = _call(lib, fake, None)
    assert rc == -1 and b"null ray batch" in msg


@pytest.mark.parametrize("field", ["orig", "dir"])
def test_shade_rays_rejects_null_rays(lib, fake, field):
    rc, msg = _call(lib, fake, _batch(**{field: None}))
    assert rc == -1 and b"null" in msg and field.encode() in msg


def test_shade_rays_rejects_a_null_output(lib, fake):
    rc, msg = _call(lib, fake, _batch(), rgb=0)
    assert rc == -1 and b"null d_rgb" in msg


@pytest.mark.parametrize("n", [0, -1, 1 << 31, -(1 << 31), 1 << 40])
def test_shade_rays_rejects_a_count_outside_the_int_range(lib, fake, n):
    rc, msg = _call(lib, fake, _batch(n=n))
    assert rc == -1 and b"n must be" in msg


@pytest.mark.parametrize("field", ["origStride", "dirStride"])
@pytest.mark.parametrize("stride", [1, 2, -1, -3, -(1 << 40)])
def test_shade_rays_rejects_a_ray_stride_below_three(lib, fake, field, stride):
    rc, msg = _call(lib, fake, _batch(**{field: stride}))
    assert rc == -1 and field.encode() in msg


@pytest.mark.parametrize("stride", [1, 2, -1, -3, -(1 << 40)])
def test_shade_rays_rejects_an_rgb_stride_below_three(lib, fake, stride):
    rc, msg = _call(lib, fake, _batch(), rgb_stride=stride)
    assert rc == -1 and b"rgbStride" in msg


def test_shade_rays_checks_do_not_depend_on_the_keys(lib, fake):
    """NULL keys are an argument, not an error: the same refusals come with and without them."""
    for key in (0, 0x7000):
        rc, msg = _call(lib, fake, _batch(key=key, n=0))
        assert rc == -1 and b"n must be" in msg


def test_camera_rays_rejects_its_argument_errors(lib, fake):
    from mobileraytracer_amd import _native
    call = lambda h, view=None, base=0, out=0x1000: lib.mrt_camera_rays_device(  # noqa: E731
        h, view, base, 1, ctypes.c_void_p(out or None), None, None, None, None)
    assert call(None) == -1 and b"null renderer" in lib.mrt_last_error()
    assert call(fake, out=0) == -1 and b"no output" in lib.mrt_last_error()
    assert call(fake, base=-1) == -1 and b"sampleBase" in lib.mrt_last_error()
    view = _native.MrtView(kind=2, a=45.0, b=45.0)  # (checked before the renderer's slots are read)
    view.up[:] = [0.0, 1.0, 0.0]
    view.lookAt[:] = [0.0, 0.0, 1.0]
    assert call(fake, ctypes.byref(view)) == -1 and b"camera kind" in lib.mrt_last_error()
    view.kind, view.a = 0, float("nan")
    assert call(fake, ctypes.byref(view)) == -1 and b"non-finite" in lib.mrt_last_error()


def test_shade_batch_struct_matches_the_header(tmp_path):
    """ctypes MrtShadeBatch has the size and the field offsets of the C mrt_shade_batch."""
    from mobileraytracer_amd import _native
    assert [f for f, _ in _native.MrtShadeBatch._fields_] == ["rays", "key"]
    src = tmp_path / "batch.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mobilert_amd.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu", sizeof(mrt_shade_batch), offsetof(mrt_shade_batch, rays),'
                   ' offsetof(mrt_shade_batch, key), sizeof(mrt_ray_batch), sizeof(mrt_view));return 0;}')
    exe = tmp_path / "batch"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_native.MrtShadeBatch), _native.MrtShadeBatch.rays.offset, _native.MrtShadeBatch.key.offset,
                   ctypes.sizeof(_native.MrtRayBatch), ctypes.sizeof(_native.MrtView)]
    assert got == [64, 0, 56, 56, 48]  # the ray batch (four pointers, three int64), then one pointer


def test_python_surface_is_there():
    import mobileraytracer_amd as m
    from mobileraytracer_amd import _native
    for name in ("shade_rays_device", "shade_rays", "camera_rays"):
        assert callable(getattr(m.Renderer, name))
    assert {"mrt_path_key", "mrt_shade_rays_device", "mrt_camera_rays_device"} <= set(_native.EXPORTED_SYMBOLS)
