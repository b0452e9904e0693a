"""Nearest-point queries without a device: the distance functions on the host (mrt_point_distance) - exact
cases, totality on degenerate input, the lemma the walk's cull rests on and the accuracy against float64 -
and the argument errors of mrt_nearest_points_device, all checked before the renderer is read."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import nearest_cases as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_BYTES = 1 << 16
FILL = b"\xa5"
FIELDS = ("kind", "index", "dist2", "point", "bary", "tests")
f32 = np.float32


def dist(kind, prims, points):
    import mobileraytracer_amd as m
    return m.point_distance(kind, prims, points)


# ---- the functions -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,case", [(N.TRIANGLE, N.exact_triangle), (N.LIGHT, N.exact_triangle),
                                       (N.PLANE, N.exact_plane), (N.SPHERE, N.exact_sphere)])
def test_exact_cases(kind, case):
    prims, pts, d2, q, uv = case()
    got = dist(kind, prims, pts)
    assert np.array_equal(got[0], d2), (got[0], d2)
    assert np.array_equal(got[1], q), (got[1], q)
    assert np.array_equal(got[2], uv), (got[2], uv)


def test_degenerate_triangles_give_finite_points_of_the_triangle():
    prims, pts = N.degenerate_triangles()
    d2, q, uv = dist(N.TRIANGLE, prims, pts)
    assert np.isfinite(d2).all() and np.isfinite(q).all() and np.isfinite(uv).all()
    assert (uv >= 0).all() and (uv.astype(np.float64).sum(1) <= 1 + 2.0 ** -23).all()
    assert (d2 >= 0).all()


@pytest.fixture(scope="module")
def lemma():
    tri, p = N.random_pairs(1 << 20, 7)
    assert len(tri) >= 10 ** 6
    d2 = dist(N.TRIANGLE, tri, p)[0]
    return tri, p, d2


def test_the_culls_lemma_holds_on_the_real_function(lemma):
    """d2 >= lb - k eps M sqrt(lb) - (k eps M)^2 against the hull of the triangle's own corners: the
    largest k seen must be at most 8, a quarter of the kernel's 32.  Measured on these 2^20 pairs: 3.07 (printed below)."""
    tri, p, d2 = lemma
    assert np.isfinite(d2).all()
    lb, M = N.hull_lb(tri, p)
    lb64, M64, d64 = lb.astype(np.float64), M.astype(np.float64), d2.astype(np.float64)
    unit = N.EPS * M64 * np.sqrt(lb64) + (N.EPS * M64) ** 2
    short = lb64 - d64
    assert (short[unit == 0] <= 0).all()
    ratio = np.where(unit > 0, short / np.where(unit > 0, unit, 1), 0.0)
    worst = int(ratio.argmax())
    print("cull lemma: %d pairs, largest (lb - d2) / (eps M sqrt(lb) + (eps M)^2) = %.3f at pair %d (lb %g, d2 %g, M %g); "
          "%d pairs with lb > 0, %d with lb > d2" % (len(tri), ratio.max(), worst, lb[worst], d2[worst], M[worst],
                                                      (lb > 0).sum(), (short > 0).sum()))
    assert (lb > 0).mean() > 0.3  # (the points are outside their triangle's box often enough to say something)
    assert ratio.max() <= 8.0
    assert N.K_KERNEL >= 4 * ratio.max()


def test_accuracy_against_float64_on_well_shaped_triangles():
    tri, p = N.random_pairs(1 << 18, 8, well_shaped=True)
    assert len(tri) > 100000
    d2 = dist(N.TRIANGLE, tri, p)[0].astype(np.float64)
    ref = N.closest_d2_f64(tri, p)
    M = N.hull_lb(tri, p)[1].astype(np.float64)
    c = N.K_KERNEL * N.EPS * M
    allowed = c * np.sqrt(d2) + c * c
    gap = np.abs(d2 - ref)
    rel = gap / np.where(allowed > 0, allowed, 1)
    print("accuracy: %d pairs, largest |d2 - float64| / (k eps M sqrt(d2) + (k eps M)^2) = %.4f" % (len(tri), rel.max()))
    assert (gap <= allowed).all()


def test_refuses_bad_pairs():
    from mobileraytracer_amd import _native
    lib = _native.lib()
    a = np.zeros(9, f32)
    ptr = a.ctypes.data_as(ctypes.c_void_p)
    for kind in (0, 5, -1):
        assert lib.mrt_point_distance(kind, ptr, ptr, 1, None, None, None) == -1 and b"kind" in lib.mrt_last_error()
    assert lib.mrt_point_distance(3, None, ptr, 1, None, None, None) == -1 and b"null" in lib.mrt_last_error()
    assert lib.mrt_point_distance(3, ptr, None, 1, None, None, None) == -1
    assert lib.mrt_point_distance(3, ptr, ptr, -1, None, None, None) == -1
    assert lib.mrt_point_distance(3, ptr, ptr, 0, None, None, None) == 0
    assert lib.mrt_point_distance(3, ptr, ptr, 1, None, None, None) == 0  # (outputs may be NULL)


# ---- argument errors ---------------------------------------------------------------------------------
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
    f = dict(point=0x1000, dist=None, src=None, stride=3, n=4)
    f.update(kw)
    return _native.MrtPointBatch(**f)


def _outputs(**kw):
    """All six fields set (the pointers stand for device memory: never dereferenced here)."""
    from mobileraytracer_amd import _native
    f = {name: 0x10000 * (k + 1) for k, name in enumerate(FIELDS)}
    f.update(kw)
    return _native.MrtNearest(**f)


def _call(lib, handle, batch, out, size=None):
    size = ctypes.sizeof(out) if size is None and out is not None else (size or 0)
    rc = lib.mrt_nearest_points_device(handle, None if batch is None else ctypes.byref(batch),
                                       None if out is None else ctypes.byref(out), size, None)
    return rc, lib.mrt_last_error()


def test_rejects_null_arguments(lib, fake):
    rc, msg = _call(lib, None, _batch(), _outputs())
    assert rc == -1 and b"mrt_nearest_points_device" in msg and b"null renderer" in msg
    rc, msg = _call(lib, fake, None, _outputs())
    assert rc == -1 and b"null point batch" in msg
    rc, msg = _call(lib, fake, _batch(), None, size=48)
    assert rc == -1 and b"null outputs" in msg
    rc, msg = _call(lib, fake, _batch(point=None), _outputs())
    assert rc == -1 and b"null point" in msg
    # ... each of them with a NULL handle too: the handle is checked first and never read
    for batch, out in ((None, _outputs()), (_batch(point=None), _outputs()), (_batch(n=0), _outputs())):
        rc, msg = _call(lib, None, batch, out)
        assert rc == -1 and b"null renderer" in msg


@pytest.mark.parametrize("size", [0, 1, 7])
def test_rejects_a_size_that_cannot_hold_kind(lib, fake, size):
    out = _outputs()
    rc = lib.mrt_nearest_points_device(fake, ctypes.byref(_batch()), ctypes.byref(out), size, None)
    assert rc == -1 and b"outSize" in lib.mrt_last_error() and b"kind" in lib.mrt_last_error()


def test_rejects_no_wanted_output_and_cuts_fields_at_the_size(lib, fake):
    rc, msg = _call(lib, fake, _batch(), _outputs(**{name: None for name in FIELDS}))
    assert rc == -1 and b"no output" in msg
    # fields beyond outSize count as null: only kind, index, dist2 are within 24 bytes
    rc, msg = _call(lib, fake, _batch(), _outputs(kind=None, index=None, dist2=None), size=24)
    assert rc == -1 and b"no output" in msg
    # ... and a field cut in half is not within it
    rc, msg = _call(lib, fake, _batch(), _outputs(kind=None, index=None, dist2=None), size=31)
    assert rc == -1 and b"no output" in msg
    rc, msg = _call(lib, fake, _batch(), _outputs(kind=None), size=8)
    assert rc == -1 and b"no output" in msg


@pytest.mark.parametrize("n", [0, -1, 1 << 31, -(1 << 31), 1 << 40])
def test_rejects_a_point_count_outside_the_int_range(lib, fake, n):
    rc, msg = _call(lib, fake, _batch(n=n), _outputs())
    assert rc == -1 and b"n must be" in msg


@pytest.mark.parametrize("stride", [1, 2, -1, -(1 << 40)])
def test_rejects_a_stride_below_three(lib, fake, stride):
    rc, msg = _call(lib, fake, _batch(stride=stride), _outputs())
    assert rc == -1 and b"stride" in msg


def test_structs_match_the_header(tmp_path):
    """ctypes MrtPointBatch / MrtNearest have the sizes and the field offsets of the C structures, and the
    symbols are exported."""
    from mobileraytracer_amd import _native
    batch = ("point", "dist", "src", "stride", "n")
    assert [f for f, _ in _native.MrtNearest._fields_] == list(FIELDS)
    assert [name for name, _, _ in _native.NEAREST_FIELDS] == list(FIELDS)
    assert [f for f, _ in _native.MrtPointBatch._fields_] == list(batch)
    src = tmp_path / "nearest.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mobilert_amd.h"\n'
                   'int main(void){printf("%zu %zu", sizeof(mrt_point_batch), sizeof(mrt_nearest));'
                   + "".join('printf(" %%zu", offsetof(mrt_point_batch, %s));' % f for f in batch)
                   + "".join('printf(" %%zu", offsetof(mrt_nearest, %s));' % f for f in FIELDS) + 'return 0;}')
    exe = tmp_path / "nearest"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_native.MrtPointBatch), ctypes.sizeof(_native.MrtNearest)] + [
        getattr(_native.MrtPointBatch, f).offset for f in batch] + [getattr(_native.MrtNearest, f).offset for f in FIELDS]
    assert got == [40, 48] + [8 * k for k in range(5)] + [8 * k for k in range(6)]
    for name in ("mrt_nearest_points_device", "mrt_point_distance", "mrt_kat_point_distance"):
        assert name in _native.EXPORTED_SYMBOLS
