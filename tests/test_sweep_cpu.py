"""Sweep queries without a device: the sweep functions on the host (mrt_sphere_sweep) - exact cases, the
two-sided contract against a float64 closed-form sweep with exact feature membership, the cull's premise - and
the argument errors of mrt_sweep_spheres_device, all checked before the renderer is read, with the ctypes
structure against the header.

Measured on these pairs (2^20 per kind, the triangles spread over the offsets 0, 100, 1024, 4096): (a) never
late holds from g = 16 for triangles and g = 8 for planes and spheres; (b) never early needs g = 38.2 for
triangles (the validation slack kSweepK = 32 plus 2^-20 r) and 6.5 for planes and spheres.  The smallest power
of two for both sides is g = 64; the tests pin 4 g = 256.  The pairs that are late at g = 1 .. 4 spread over the
decades of L / r (0.1 .. 100) as the pairs themselves do.  The function hits 0.769 of the triangle pairs (the
float64 yardstick 0.707: a third of the sweeps graze within 1e-7 .. 1e-1 of r), 0.743 of the plane pairs and
0.772 of the sphere pairs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sweep_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_BYTES = 1 << 16
FILL = b"\xa5"
FIELDS = ("hit", "kind", "index", "t", "centre", "point", "bary", "tests")
f32 = np.float32
INF, NAN = np.inf, np.nan


def sweep(kind, prim, ray):
    import mobileraytracer_amd as m
    hit, t, c, q, uv = m.sphere_sweep(kind, np.array([prim], f32), np.array([ray], f32))
    return int(hit[0]), float(t[0]), tuple(map(float, c[0])), tuple(map(float, q[0])), tuple(map(float, uv[0]))


MISS = (0, INF, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0))

# ---- exact cases -----------------------------------------------------------------------------------------
RIGHT = (0, 0, 0, 4, 0, 0, 0, 4, 0)  # A, AB, AC: the right triangle in z = 0 with legs of 4
SEGMENT = (0, 0, 0, 4, 0, 0, 0, 0, 0)  # AC = 0
POINT = (1, 2, 3, 0, 0, 0, 0, 0, 0)  # AB = AC = 0
TRIANGLE_CASES = [  # name, triangle, (o, d, r), (hit, t, centre, point, bary)
    ("dropped on the face", RIGHT, (1, 1, 5, 0, 0, -1, 1), (1, 4.0, (1, 1, 1), (1, 1, 0), (0.25, 0.25))),
    ("dropped on the face from below, d not unit", RIGHT, (1, 1, -9, 0, 0, 2, 1), (1, 4.0, (1, 1, -1), (1, 1, 0), (0.25, 0.25))),
    ("dropped on an edge (3-4-5)", RIGHT, (2, -3, 10, 0, 0, -1, 5), (1, 6.0, (2, -3, 4), (2, 0, 0), (0.5, 0))),
    ("dropped on a corner", RIGHT, (6, -2, 5, 0, 0, -1, 3), (1, 4.0, (6, -2, 1), (4, 0, 0), (1, 0))),
    ("a start in contact", RIGHT, (1, 1, 0.5, 0, 0, -1, 1), (1, 0.0, (1, 1, 0.5), (1, 1, 0), (0.25, 0.25))),
    ("a start touching exactly", RIGHT, (1, 1, 1, 0, 0, 1, 1), (1, 0.0, (1, 1, 1), (1, 1, 0), (0.25, 0.25))),
    ("moving away", RIGHT, (1, 1, 5, 0, 0, 1, 1), MISS),
    ("passing beside", RIGHT, (9, 9, 5, 0, 0, -1, 1), MISS),
    ("d = 0 touching", RIGHT, (1, 1, 0.5, 0, 0, 0, 1), (1, 0.0, (1, 1, 0.5), (1, 1, 0), (0.25, 0.25))),
    ("d = 0 not touching", RIGHT, (1, 1, 5, 0, 0, 0, 1), MISS),
    ("r = 0: a moving point", RIGHT, (1, 1, 5, 0, 0, -1, 0), (1, 5.0, (1, 1, 0), (1, 1, 0), (0.25, 0.25))),
    ("AC = 0: swept as a segment", SEGMENT, (2, -3, 10, 0, 0, -1, 5), (1, 6.0, (2, -3, 4), (2, 0, 0), (0.5, 0))),
    ("AC = 0: past the segment's end onto its corner", SEGMENT, (6, -2, 5, 0, 0, -1, 3), (1, 4.0, (6, -2, 1), (4, 0, 0), (1, 0))),
    ("AB = AC = 0: swept as a point", POINT, (1, 2, 10, 0, 0, -1, 2), (1, 5.0, (1, 2, 5), (1, 2, 3), (0, 0))),
    ("AB = AC = 0: passing the point", POINT, (1, 5, 10, 0, 0, -1, 2), MISS),
]


@pytest.mark.parametrize("name,tri,ray,want", TRIANGLE_CASES, ids=[c[0] for c in TRIANGLE_CASES])
def test_exact_triangle_cases(name, tri, ray, want):
    for kind in (C.TRIANGLE, C.LIGHT):
        assert sweep(kind, tri, ray) == want
    ex = C.first_contact_f64(C.TRIANGLE, np.array([tri], f32), np.array([ray], f32))[0]  # (the yardstick agrees)
    assert ex == (want[1] if want[0] else INF)


def test_exact_plane_cases_from_both_sides():
    plane = (0, 0, 1, 7, -3, 2)  # z = 2
    assert sweep(C.PLANE, plane, (0, 0, 6, 0, 0, -2, 1)) == (1, 1.5, (0, 0, 3), (0, 0, 2), (0, 0))
    assert sweep(C.PLANE, plane, (0, 0, -4, 0, 0, 1, 2)) == (1, 4.0, (0, 0, 0), (0, 0, 2), (0, 0))
    assert sweep(C.PLANE, plane, (5, 5, 2.5, 1, 0, 0, 1)) == (1, 0.0, (5, 5, 2.5), (5, 5, 2), (0, 0))  # starts in contact
    assert sweep(C.PLANE, plane, (0, 0, 6, 0, 0, 1, 1)) == MISS  # moving away
    assert sweep(C.PLANE, plane, (0, 0, 6, 1, 1, 0, 1)) == MISS  # parallel
    assert sweep(C.PLANE, plane, (0, 0, 6, 0, 0, 0, 1)) == MISS  # d = 0


def test_exact_sphere_cases_from_outside_and_inside():
    sphere = (1, 1, 1, 4)  # radius 2 about (1, 1, 1)
    assert sweep(C.SPHERE, sphere, (1, 1, 9, 0, 0, -1, 2)) == (1, 4.0, (1, 1, 5), (1, 1, 3), (0, 0))
    assert sweep(C.SPHERE, sphere, (1, 1, 1, 0, 0, 1, 1)) == (1, 1.0, (1, 1, 2), (1, 1, 3), (0, 0))  # from the centre outwards
    assert sweep(C.SPHERE, sphere, (1, 1, 2.5, 1, 0, 0, 1)) == (1, 0.0, (1, 1, 2.5), (1, 1, 3), (0, 0))  # touching from within
    assert sweep(C.SPHERE, sphere, (1, 1, 9, 0, 0, 1, 2)) == MISS  # moving away
    assert sweep(C.SPHERE, sphere, (9, 1, 9, 0, 0, -1, 2)) == MISS  # passing beside
    assert sweep(C.SPHERE, sphere, (1, 1, 1, 0, 0, 0, 1)) == MISS  # d = 0 inside, not touching


def test_invalid_input_accepts_nothing():
    good = (1, 1, 5, 0, 0, -1, 1)
    prims = ((C.TRIANGLE, RIGHT), (C.PLANE, (0, 0, 1, 0, 0, 0)), (C.SPHERE, (1, 1, 0, 4)))
    for kind, prim in prims:
        assert sweep(kind, prim, good)[0] == 1
    for bad in (NAN, INF, -INF):
        for slot in range(7):
            ray = list(good)
            ray[slot] = bad
            for kind, prim in prims:
                assert sweep(kind, prim, ray) == MISS, (kind, slot, bad)
    for kind, prim in prims:
        assert sweep(kind, prim, good[:6] + (-1,)) == MISS
        assert sweep(kind, prim, good[:6] + (-1e-30,)) == MISS
    for slot in range(9):  # a non-finite corner is never accepted
        for bad in (NAN, INF):
            tri = list(RIGHT)
            tri[slot] = bad
            assert sweep(C.TRIANGLE, tri, good)[0] == 0, (slot, bad)


# ---- the contract ------------------------------------------------------------------------------------------
KINDS = (C.TRIANGLE, C.PLANE, C.SPHERE)


_PAIRS = {}


def _pairs(kind):
    """The kind's 2^20 pairs with the function's answers and the yardstick's times, made once."""
    import mobileraytracer_amd as m
    if kind not in _PAIRS:
        prims, rays = C.PAIRS[kind](1 << 20, 11)
        hit, t, centre, _, _ = m.sphere_sweep(kind, prims, rays)
        _PAIRS[kind] = (kind, prims, rays, hit != 0, t, centre, C.first_contact_f64(kind, prims, rays))
    return _PAIRS[kind]


@pytest.fixture(scope="module", params=KINDS, ids=["triangles", "planes", "spheres"])
def pairs(request):
    return _pairs(request.param)


def test_the_hit_share_is_between_20_and_80_percent(pairs):
    kind, prims, rays, hit, t, centre, exact = pairs
    print("kind %d: the function hits %.3f, float64 %.3f; t = 0: %.3f" % (kind, hit.mean(), np.isfinite(exact).mean(),
                                                                      (hit & (t == 0)).mean()))
    assert 0.20 <= hit.mean() <= 0.80
    assert 0.20 <= np.isfinite(exact).mean() <= 0.80


def test_never_late(pairs):
    """(a): the returned t (a miss: +inf) is at most the exact first-contact time of the sphere shrunk to
    r - 4 g eps M, M with the centre at the exact contact of the unshrunk sphere."""
    kind, prims, rays, hit, t, centre, exact = pairs
    r = rays[:, 6].astype(np.float64)
    M = C.scale_of(kind, prims, rays, C.centre64(rays, np.where(np.isfinite(exact), exact, 0.0)))
    got = np.where(hit, t.astype(np.float64), INF)
    L = np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1) * np.where(np.isfinite(exact), exact, NAN)
    with np.errstate(invalid="ignore", divide="ignore"):
        decade = np.floor(np.log10(L / r))
    for g in (C.G / 16, C.G / 4):
        late = got > C.first_contact_f64(kind, prims, rays, r - g * C.EPS * M)
        print("kind %d: g = %g leaves %d late, per decade of L / r %s" % (
            kind, g, int(late.sum()), {int(k): int((late & (decade == k)).sum()) for k in (-1, 0, 1, 2)}))
    late = got > C.first_contact_f64(kind, prims, rays, r - 4 * C.G * C.EPS * M)
    assert not late.any(), (int(late.sum()), prims[late][0], rays[late][0])


def test_never_early(pairs):
    """(b): at a hit the exact distance from the reported centre to the primitive is at most r + 4 g eps M."""
    kind, prims, rays, hit, t, centre, exact = pairs
    r = rays[:, 6].astype(np.float64)
    c = centre.astype(np.float64)
    need = np.where(hit, (C.distance_f64(kind, prims, c) - r) / (C.EPS * C.scale_of(kind, prims, rays, c)), -INF)
    print("kind %d: the largest g a hit needs is %.2f" % (kind, need.max()))
    early = need > 4 * C.G
    assert not early.any(), (int(early.sum()), prims[early][0], rays[early][0])


def test_a_hit_s_centre_is_within_the_cull_radius_of_the_hull():
    """The cull's premise: the reported centre lies within the header's R of the triangle's float32 hull box on
    every axis (R from the box itself: no larger than from any box above it)."""
    kind, prims, rays, hit, t, centre, exact = _pairs(C.TRIANGLE)
    P = C.OC.corners32(prims)
    lo, hi = np.minimum(np.minimum(P[0], P[1]), P[2]), np.maximum(np.maximum(P[0], P[1]), P[2])
    assert lo.dtype == f32
    lo, hi, c = lo.astype(np.float64), hi.astype(np.float64), centre.astype(np.float64)
    r = rays[:, 6].astype(np.float64)
    mr = np.maximum(np.maximum(np.abs(lo).max(1), np.abs(hi).max(1)), np.maximum(np.abs(rays[:, :3]).max(1), r))
    R = C.cull_radius(r, mr)[:, None]
    out = hit & ((c < lo - R) | (c > hi + R)).any(1)
    assert not out.any(), (int(out.sum()), prims[out][0], rays[out][0])


def test_a_light_is_a_triangle():
    import mobileraytracer_amd as m
    prims, rays = C.triangle_sweeps(1 << 12, 3)
    a, b = m.sphere_sweep(C.LIGHT, prims, rays), m.sphere_sweep(C.TRIANGLE, prims, rays)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


def test_the_constants_are_the_header_s():
    text = open(os.path.join(REPO, "mobileraytracer_amd", "csrc", "mrt_sweep.hpp")).read()
    assert "constexpr float kSweepK = %.1fF;" % C.SWEEP_K in text
    assert "constexpr float kSweepG = %.1fF;" % C.G in text
    near = open(os.path.join(REPO, "mobileraytracer_amd", "csrc", "mrt_nearest.hpp")).read()
    assert "constexpr float kNearestK = %.1fF;" % C.NEAREST_K in near


# ---- the interface -------------------------------------------------------------------------------------------
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
    """All eight fields set (the pointers stand for device memory: never dereferenced here)."""
    from mobileraytracer_amd import _native
    f = {name: 0x10000 * (k + 1) for k, name in enumerate(FIELDS)}
    f.update(kw)
    return _native.MrtSweeps(**f)


def _call(lib, handle, batch, out, radius=0x3000, size=None):
    size = ctypes.sizeof(out) if size is None and out is not None else (size or 0)
    rc = lib.mrt_sweep_spheres_device(handle, None if batch is None else ctypes.byref(batch), radius,
                                      None if out is None else ctypes.byref(out), size, None)
    return rc, lib.mrt_last_error()


def test_rejects_null_arguments(lib, fake):
    rc, msg = _call(lib, None, _batch(), _outputs())
    assert rc == -1 and b"mrt_sweep_spheres_device" in msg and b"null renderer" in msg
    rc, msg = _call(lib, fake, None, _outputs())
    assert rc == -1 and b"null ray batch" in msg
    rc, msg = _call(lib, fake, _batch(), None, size=64)
    assert rc == -1 and b"null outputs" in msg
    rc, msg = _call(lib, fake, _batch(), _outputs(), radius=None)
    assert rc == -1 and b"null d_radius" in msg
    for kw in ({"orig": None}, {"dir": None}):
        rc, msg = _call(lib, fake, _batch(**kw), _outputs())
        assert rc == -1 and b"null orig / dir" in msg
    # ... each of them with a NULL handle too: the handle is checked first and never read
    for batch, out, radius in ((None, _outputs(), 0x3000), (_batch(orig=None), _outputs(), 0x3000),
                               (_batch(n=0), _outputs(), 0x3000), (_batch(), _outputs(), None)):
        rc, msg = _call(lib, None, batch, out, radius=radius)
        assert rc == -1 and b"null renderer" in msg


@pytest.mark.parametrize("size", [0, 1, 7])
def test_rejects_a_size_that_cannot_hold_hit(lib, fake, size):
    out = _outputs()
    rc = lib.mrt_sweep_spheres_device(fake, ctypes.byref(_batch()), 0x3000, ctypes.byref(out), size, None)
    assert rc == -1 and b"outSize" in lib.mrt_last_error() and b"hit" in lib.mrt_last_error()


def test_rejects_no_wanted_output_and_cuts_fields_at_the_size(lib, fake):
    rc, msg = _call(lib, fake, _batch(), _outputs(**{name: None for name in FIELDS}))
    assert rc == -1 and b"no output" in msg
    # fields beyond outSize count as null: only hit, kind, index are within 24 bytes
    rc, msg = _call(lib, fake, _batch(), _outputs(hit=None, kind=None, index=None), size=24)
    assert rc == -1 and b"no output" in msg
    # ... and a field cut in half is not within it
    rc, msg = _call(lib, fake, _batch(), _outputs(hit=None, kind=None, index=None), size=31)
    assert rc == -1 and b"no output" in msg
    rc, msg = _call(lib, fake, _batch(), _outputs(hit=None), size=8)
    assert rc == -1 and b"no output" in msg


@pytest.mark.parametrize("n", [0, -1, 1 << 31, -(1 << 31), 1 << 40])
def test_rejects_a_ray_count_outside_the_int_range(lib, fake, n):
    rc, msg = _call(lib, fake, _batch(n=n), _outputs())
    assert rc == -1 and b"n must be" in msg


@pytest.mark.parametrize("stride", [1, 2, -1, -(1 << 40)])
def test_rejects_a_stride_below_three(lib, fake, stride):
    for kw in ({"origStride": stride}, {"dirStride": stride}):
        rc, msg = _call(lib, fake, _batch(**kw), _outputs())
        assert rc == -1 and b"Stride" in msg


def test_sphere_sweep_checks_its_arguments(lib):
    ptr = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    for kind in (0, 5, -1):
        assert lib.mrt_sphere_sweep(kind, ptr, ptr, 1, ptr, ptr, ptr, ptr, ptr) == -1 and b"kind" in lib.mrt_last_error()
    assert lib.mrt_sphere_sweep(3, None, ptr, 1, ptr, ptr, ptr, ptr, ptr) == -1 and b"null" in lib.mrt_last_error()
    assert lib.mrt_sphere_sweep(3, ptr, None, 1, ptr, ptr, ptr, ptr, ptr) == -1
    assert lib.mrt_sphere_sweep(3, ptr, ptr, -1, ptr, ptr, ptr, ptr, ptr) == -1
    assert lib.mrt_sphere_sweep(3, ptr, ptr, 0, ptr, ptr, ptr, ptr, ptr) == 0
    assert lib.mrt_sphere_sweep(3, ptr, ptr, 1, None, None, None, None, None) == 0  # (a NULL output is not written)


def test_struct_matches_the_header(tmp_path):
    """ctypes MrtSweeps has the size and the field offsets of the C structure, mrt_ray_batch is unchanged, and
    the symbols are exported."""
    from mobileraytracer_amd import _native
    batch = ("orig", "dir", "dist", "src", "origStride", "dirStride", "n")
    assert [f for f, _ in _native.MrtSweeps._fields_] == list(FIELDS)
    assert [f for f, _ in _native.MrtRayBatch._fields_] == list(batch)
    assert {name: w for name, _, w in _native.SWEEP_FIELDS} == C.WIDTHS
    src = tmp_path / "sweeps.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mobilert_amd.h"\n'
                   'int main(void){printf("%zu %zu", sizeof(mrt_sweeps), sizeof(mrt_ray_batch));'
                   + "".join('printf(" %%zu", offsetof(mrt_sweeps, %s));' % f for f in FIELDS)
                   + "".join('printf(" %%zu", offsetof(mrt_ray_batch, %s));' % f for f in batch) + 'return 0;}')
    exe = tmp_path / "sweeps"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_native.MrtSweeps), ctypes.sizeof(_native.MrtRayBatch)] + [
        getattr(_native.MrtSweeps, f).offset for f in FIELDS] + [getattr(_native.MrtRayBatch, f).offset for f in batch]
    assert got == [64, 56] + [8 * k for k in range(8)] + [8 * k for k in range(7)]
    for name in ("mrt_sweep_spheres_device", "mrt_sphere_sweep", "mrt_kat_sphere_sweep"):
        assert name in _native.EXPORTED_SYMBOLS
