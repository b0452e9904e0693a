"""mrt_render_views / mrt_render_views_device without a device: the argument errors that are checked
before any device work, and the ctypes mirror of mrt_view."""
import ctypes
import math
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _view(kind=0, position=(0.0, 0.0, -3.4), look_at=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), a=45.0, b=45.0):
    from mobileraytracer_amd import _native
    v = _native.MrtView()
    v.kind = kind
    v.position[:] = position
    v.lookAt[:] = look_at
    v.up[:] = up
    v.a, v.b = a, b
    return v


@pytest.fixture(scope="module")
def lib(native_lib_path):
    from mobileraytracer_amd import _native
    return _native.load_library(native_lib_path)


def _both(lib, handle, views, n, out):
    """(status, message) of the host and of the device entry point for the same arguments."""
    res = []
    rc = lib.mrt_render_views(handle, views, n, out)
    res.append((rc, lib.mrt_last_error()))
    rc = lib.mrt_render_views_device(handle, views, n, out, None, None)
    res.append((rc, lib.mrt_last_error()))
    return res


def test_views_reject_null_handles(lib):
    from mobileraytracer_amd import _native
    views = (_native.MrtView * 2)(_view(), _view(1))
    out = (ctypes.c_int32 * 16)()
    for rc, msg in _both(lib, None, views, 2, out):
        assert rc == -1 and b"null" in msg
    # (the views are checked before the renderer is read: an opaque block stands in for it)
    fake = ctypes.create_string_buffer(1 << 16)
    for rc, msg in _both(lib, fake, None, 2, out):
        assert rc == -1 and b"null" in msg


@pytest.mark.parametrize("n", [0, -1, -(1 << 31)])
def test_views_reject_a_count_below_one(lib, n):
    from mobileraytracer_amd import _native
    views = (_native.MrtView * 1)(_view())
    out = (ctypes.c_int32 * 16)()
    fake = ctypes.create_string_buffer(1 << 16)
    for rc, msg in _both(lib, fake, views, n, out):
        assert rc == -1 and b"nViews" in msg


@pytest.mark.parametrize("kind", [-1, 2, 7])
def test_views_reject_a_camera_kind_outside_0_1(lib, kind):
    from mobileraytracer_amd import _native
    views = (_native.MrtView * 2)(_view(), _view(kind))
    out = (ctypes.c_int32 * 16)()
    fake = ctypes.create_string_buffer(1 << 16)
    for rc, msg in _both(lib, fake, views, 2, out):
        assert rc == -1 and b"camera kind" in msg


@pytest.mark.parametrize("field", ["position", "lookAt", "up", "a", "b"])
@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_views_reject_non_finite_fields(lib, field, bad):
    from mobileraytracer_amd import _native
    v = _view(1)
    if field in ("a", "b"):
        setattr(v, field, bad)
    else:
        getattr(v, field)[1] = bad
    views = (_native.MrtView * 3)(_view(), _view(), v)
    out = (ctypes.c_int32 * 16)()
    fake = ctypes.create_string_buffer(1 << 16)
    for rc, msg in _both(lib, fake, views, 3, out):
        assert rc == -1 and b"non-finite" in msg and b"view 2" in msg


def test_views_reject_no_output(lib):
    from mobileraytracer_amd import _native
    views = (_native.MrtView * 1)(_view())
    fake = ctypes.create_string_buffer(1 << 16)
    for rc, msg in _both(lib, fake, views, 1, None):
        assert rc == -1 and b"no output" in msg


def test_view_struct_matches_the_header(tmp_path):
    """ctypes MrtView has the size and the field offsets of the C mrt_view."""
    from mobileraytracer_amd import _native
    fields = ("kind", "position", "lookAt", "up", "a", "b")
    src = tmp_path / "view.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mobilert_amd.h"\n'
                   'int main(void){printf("%zu", sizeof(mrt_view));'
                   + "".join('printf(" %%zu", offsetof(mrt_view, %s));' % f for f in fields) + 'return 0;}')
    exe = tmp_path / "view"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_native.MrtView)] + [getattr(_native.MrtView, f).offset for f in fields]
    assert got[0] == 48
