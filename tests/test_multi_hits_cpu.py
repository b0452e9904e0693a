"""Multi-hit queries without a device: the argument errors of mrt_cast_multi_hits_device, all checked
before the renderer is read (an opaque block stands in for it and must stay untouched), and the ctypes
mirror of mrt_multi_hits against the header."""
import ctypes
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_BYTES = 1 << 16
FILL = b"\xa5"
FIELDS = ("count", "kind", "index", "t", "bary")


@pytest.fixture(scope="module")
def lib(native_lib_path):
    from mobileraytracer_amd import _native
    return _native.load_library(native_lib_path)


@pytest.fixture()
def fake():
    """An opaque block standing in for the renderer: never dereferenced, never written (checked after
    each test)."""
    block = ctypes.create_string_buffer(FILL * FAKE_BYTES, FAKE_BYTES)
    yield block
    assert block.raw == FILL * FAKE_BYTES


def _batch(**kw):
    from mobileraytracer_amd import _native
    f = dict(orig=0x1000, dir=0x2000, dist=None, src=None, origStride=3, dirStride=3, n=4)
    f.update(kw)
    return _native.MrtRayBatch(**f)


def _outputs(**kw):
    """All five fields set (the pointers stand for device memory: never dereferenced here)."""
    from mobileraytracer_amd import _native
    f = {name: 0x10000 * (k + 1) for k, name in enumerate(FIELDS)}
    f.update(kw)
    return _native.MrtMultiHits(**f)


def _call(lib, handle, batch, out, k=4, size=None):
    size = ctypes.sizeof(out) if size is None and out is not None else (size or 0)
    rc = lib.mrt_cast_multi_hits_device(handle, None if batch is None else ctypes.byref(batch), k,
                                        None if out is None else ctypes.byref(out), size, None)
    return rc, lib.mrt_last_error()


def test_rejects_null_arguments(lib, fake):
    rc, msg = _call(lib, None, _batch(), _outputs())
    assert rc == -1 and b"mrt_cast_multi_hits_device" in msg and b"null renderer" in msg
    rc, msg = _call(lib, fake, None, _outputs())
    assert rc == -1 and b"null ray batch" in msg
    rc, msg = _call(lib, fake, _batch(), None, size=40)
    assert rc == -1 and b"null multi hits" in msg
    for field in ("orig", "dir"):
        rc, msg = _call(lib, fake, _batch(**{field: None}), _outputs())
        assert rc == -1 and b"null" in msg and field.encode() in msg


@pytest.mark.parametrize("k", [0, -1, 17, 1 << 20, -(1 << 31)])
def test_rejects_a_k_outside_1_to_16(lib, fake, k):
    rc, msg = _call(lib, fake, _batch(), _outputs(), k=k)
    assert rc == -1 and b"K must be 1 .. 16" in msg


@pytest.mark.parametrize("size", [0, 1, 7])
def test_rejects_a_size_that_cannot_hold_count(lib, fake, size):
    out = _outputs()
    rc = lib.mrt_cast_multi_hits_device(fake, ctypes.byref(_batch()), 4, ctypes.byref(out), size, None)
    assert rc == -1 and b"outSize" in lib.mrt_last_error() and b"count" in lib.mrt_last_error()


def test_rejects_no_wanted_output_and_cuts_fields_at_the_size(lib, fake):
    rc, msg = _call(lib, fake, _batch(), _outputs(**{name: None for name in FIELDS}))
    assert rc == -1 and b"no output" in msg
    # fields beyond outSize count as null: only count, kind, index are within 24 bytes
    rc, msg = _call(lib, fake, _batch(), _outputs(count=None, kind=None, index=None), size=24)
    assert rc == -1 and b"no output" in msg
    # ... and a field cut in half is not within it
    rc, msg = _call(lib, fake, _batch(), _outputs(count=None, kind=None, index=None), size=31)
    assert rc == -1 and b"no output" in msg
    rc, msg = _call(lib, fake, _batch(), _outputs(count=None), size=8)
    assert rc == -1 and b"no output" in msg


@pytest.mark.parametrize("n", [0, -1, 1 << 31, -(1 << 31), 1 << 40])
def test_rejects_a_ray_count_outside_the_int_range(lib, fake, n):
    rc, msg = _call(lib, fake, _batch(n=n), _outputs())
    assert rc == -1 and b"n must be" in msg


@pytest.mark.parametrize("field", ["origStride", "dirStride"])
@pytest.mark.parametrize("stride", [1, 2, -1, -(1 << 40)])
def test_rejects_a_stride_below_three(lib, fake, field, stride):
    rc, msg = _call(lib, fake, _batch(**{field: stride}), _outputs())
    assert rc == -1 and field.encode() in msg


def test_multi_hits_struct_matches_the_header(tmp_path):
    """ctypes MrtMultiHits has the size and the field offsets of the C mrt_multi_hits, the K limit is
    the header's, and the symbol is exported."""
    from mobileraytracer_amd import _native
    assert [f for f, _ in _native.MrtMultiHits._fields_] == list(FIELDS)
    assert [name for name, _, _ in _native.MULTI_HIT_FIELDS] == list(FIELDS)
    src = tmp_path / "multi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mobilert_amd.h"\n'
                   'int main(void){printf("%d %zu", MRT_MULTI_HITS_MAX, sizeof(mrt_multi_hits));'
                   + "".join('printf(" %%zu", offsetof(mrt_multi_hits, %s));' % f for f in FIELDS) + 'return 0;}')
    exe = tmp_path / "multi"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [_native.MULTI_HITS_MAX, ctypes.sizeof(_native.MrtMultiHits)] + [
        getattr(_native.MrtMultiHits, f).offset for f in FIELDS]
    assert got == [16, 40] + [8 * k for k in range(5)]
    assert "mrt_cast_multi_hits_device" in _native.EXPORTED_SYMBOLS
