"""mrt_cast_rays_device without a device: the argument errors that are checked before any device
work, and the ctypes mirror of mrt_ray_batch."""
import ctypes
import os
import subprocess

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
    """An opaque block standing in for the renderer: the batch and the outputs are checked before
    the renderer is read, so it is never dereferenced (and never written: checked after each call)."""
    block = ctypes.create_string_buffer(FILL * FAKE_BYTES, FAKE_BYTES)
    yield block
    assert block.raw == FILL * FAKE_BYTES


def _batch(**kw):
    """A well-formed batch of 4 rays (the pointers stand for device memory: never dereferenced on
    the paths tested here), with the given fields replaced."""
    from mobileraytracer_amd import _native
    f = dict(orig=0x1000, dir=0x2000, dist=0x3000, src=None, origStride=3, dirStride=3, n=4)
    f.update(kw)
    return _native.MrtRayBatch(**f)


def _call(lib, handle, batch, any_hit=0, kind=0x4000, index=0x5000, t=0x6000):
    rc = lib.mrt_cast_rays_device(handle, None if batch is None else ctypes.byref(batch), any_hit,
                                  ctypes.c_void_p(kind or None), ctypes.c_void_p(index or None),
                                  ctypes.c_void_p(t or None), None)
    return rc, lib.mrt_last_error()


def test_cast_rays_rejects_a_null_handle(lib):
    rc, msg = _call(lib, None, _batch())
    assert rc == -1 and b"null renderer" in msg


def test_cast_rays_rejects_a_null_batch(lib, fake):
    rc, msg = _call(lib, fake, None)
    assert rc == -1 and b"null ray batch" in msg


@pytest.mark.parametrize("field", ["orig", "dir"])
@pytest.mark.parametrize("any_hit", [0, 1])
def test_cast_rays_rejects_null_rays(lib, fake, field, any_hit):
    rc, msg = _call(lib, fake, _batch(**{field: None}), any_hit)
    assert rc == -1 and b"null" in msg and field.encode() in msg


def test_cast_rays_rejects_any_hit_without_dist(lib, fake):
    rc, msg = _call(lib, fake, _batch(dist=None), 1)
    assert rc == -1 and b"dist" in msg


@pytest.mark.parametrize("n", [0, -1, 1 << 31, -(1 << 31), 1 << 40])
def test_cast_rays_rejects_a_count_outside_the_int_range(lib, fake, n):
    rc, msg = _call(lib, fake, _batch(n=n))
    assert rc == -1 and b"n must be" in msg


@pytest.mark.parametrize("field", ["origStride", "dirStride"])
@pytest.mark.parametrize("stride", [1, 2, -1, -3, -(1 << 40)])
def test_cast_rays_rejects_a_stride_below_three(lib, fake, field, stride):
    rc, msg = _call(lib, fake, _batch(**{field: stride}))
    assert rc == -1 and field.encode() in msg


def test_cast_rays_rejects_no_wanted_output(lib, fake):
    rc, msg = _call(lib, fake, _batch(), 0, kind=0, index=0, t=0)
    assert rc == -1 and b"no output" in msg
    # any hit writes d_kind only: d_index and d_t are not wanted outputs
    rc, msg = _call(lib, fake, _batch(), 1, kind=0)
    assert rc == -1 and b"no output" in msg and b"d_kind" in msg


def test_ray_batch_struct_matches_the_header(tmp_path):
    """ctypes MrtRayBatch has the size and the field offsets of the C mrt_ray_batch."""
    from mobileraytracer_amd import _native
    fields = ("orig", "dir", "dist", "src", "origStride", "dirStride", "n")
    assert [f for f, _ in _native.MrtRayBatch._fields_] == list(fields)
    src = tmp_path / "batch.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mobilert_amd.h"\n'
                   'int main(void){printf("%zu", sizeof(mrt_ray_batch));'
                   + "".join('printf(" %%zu", offsetof(mrt_ray_batch, %s));' % f for f in fields) + 'return 0;}')
    exe = tmp_path / "batch"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_native.MrtRayBatch)] + [getattr(_native.MrtRayBatch, f).offset for f in fields]
    assert got == [56, 0, 8, 16, 24, 32, 40, 48]  # four pointers and three int64
