"""Triangle overlap queries without a device: the overlap functions of a query triangle on the host
(mrt_triangle_overlap) - exact cases, the contract against float64 yardsticks (no intersecting pair lost; every
acceptance explained by a distance of 4 g eps M), the cull's premise - and the argument errors of
mrt_overlap_triangles_device, all checked before the renderer is read, with the ctypes structures against the
header.

Measured on these pairs: the smallest power of two g for which no accepted pair is farther apart than g eps M
(float64, on the stored float32 corners).  The contract's pairs, 2^20 per offset: 32 at every offset, 0, 100, 1024 and
4096 (at offset 0 three pairs need more than 1); float64 accepts 17.2 % of them at every offset, the function
17.2, 17.2, 17.3 and 17.7 %.  The families of 2^16 pairs: 32 for exactly coplanar pairs, 32 for query segments, 64 for query points,
16 for planes, 64 for spheres; pairs sharing a corner or an edge bit for bit all intersect and are all accepted.
kTriOverlapG = 64, and the tests pin 4 g = 256."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import triangle_overlap_cases as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_BYTES = 1 << 16
FILL = b"\xa5"
FIELDS = ("any", "count", "kind", "index", "tests")
f32 = np.float32
INF, NAN = np.inf, np.nan


def overlap(kind, prims, tris):
    import mobileraytracer_amd as m
    return m.triangle_overlap(kind, np.array(prims, f32), np.array(tris, f32))


# ---- exact cases -----------------------------------------------------------------------------------------
RIGHT = (0, 0, 0, 4, 0, 0, 0, 4, 0)  # A, AB, AC: the right triangle in z = 0 with legs of 4
WIDE = (-4, -4, 0, 8, 0, 0, 4, 8, 0)  # corners (-4, -4, 0), (4, -4, 0), (0, 4, 0)
SKEW = (-4, 0, 0, 8, 0, 0, 4, -4, -2)  # corners (-4, 0, 0), (4, 0, 0), (0, -4, -2)
S20 = 2.0 ** -20
TRIANGLE_CASES = [  # name, scene triangle (A, AB, AC), query triangle (a, b, c), expected
    ("crossing triangles", RIGHT, (2, -2, -1, 2, 2, -1, 2, 0, 3), 1),
    ("piercing the face, no edge crossing an edge", (-64, -64, 0, 256, 0, 0, 0, 256, 0), (1, 1, -1, 2, 1, 1, 1, 2, 1), 1),
    ("a shared corner only", RIGHT, (4, 0, 0, 6, 0, 1, 6, 1, -1), 1),
    ("a shared edge", RIGHT, (0, 0, 0, 4, 0, 0, 2, -2, 3), 1),
    ("coplanar overlapping", RIGHT, (1, 1, 0, 5, 1, 0, 1, 5, 0), 1),
    ("coplanar apart, separated only by an in-plane edge normal", RIGHT, (3, 3, 0, 5, 3, 0, 3, 5, 0), 0),
    ("parallel planes 2^-20 apart", RIGHT, (1, 1, S20, 2, 1, S20, 1, 2, S20), 0),
    ("tilted 2^-20 above the face", RIGHT, (1, 1, S20, 2, 1, 2 * S20, 1, 2, 1), 0),
    ("separated only by one edge cross product", SKEW, (0, -3, 4, 0, 4, -3, 1, 3, 3), 0),
    ("the same pair moved together along that axis", SKEW, (0, -4, 3, 0, 3, -4, 1, 2, 2), 1),
    ("the same triangle", RIGHT, (0, 0, 0, 4, 0, 0, 0, 4, 0), 1),
    ("the same triangle, corners rotated", RIGHT, (0, 4, 0, 0, 0, 0, 4, 0, 0), 1),
    # query segments (two equal corners)
    ("a segment through the face", RIGHT, (1, 1, -1, 1, 1, 1, 1, 1, 1), 1),
    ("a segment ending in the face", RIGHT, (1, 1, 0, 1, 1, 0, 1, 1, 3), 1),
    ("a segment through an edge", RIGHT, (2, 0, -1, 2, 0, 1, 2, 0, 1), 1),
    ("a segment touching an edge with its end", RIGHT, (2, 0, 0, 2, -3, 2, 2, 0, 0), 1),
    ("a coplanar segment crossing the triangle", RIGHT, (-1, 1, 0, 5, 1, 0, 5, 1, 0), 1),
    ("a coplanar segment beside the triangle", RIGHT, (3, 3, 0, 5, 3, 0, 5, 3, 0), 0),
    ("a segment passing above an edge", RIGHT, (2, -1, 1, 2, 1, 1, 2, 1, 1), 0),
    # query points (three equal corners)
    ("a point on a corner", RIGHT, (4, 0, 0) * 3, 1),
    ("a point in the face", RIGHT, (1, 1, 0) * 3, 1),
    ("a point on the hypotenuse", RIGHT, (2, 2, 0) * 3, 1),
    ("a point off the face", RIGHT, (1, 1, 0.5) * 3, 0),
    ("a coplanar point beyond the hypotenuse", RIGHT, (3, 3, 0) * 3, 0),
    # degenerate scene triangles
    ("AC = 0: a scene segment through the query's face", (-2, -2, -2, 4, 4, 4, 0, 0, 0), (-4, -4, 0, 4, -4, 0, 0, 4, 0), 1),
    ("AC = 0: a scene segment beside the query", (3, 3, -1, 0, 0, 2, 0, 0, 0), (-4, -4, 0, 4, -4, 0, 0, 4, 0), 0),
    ("AB = AC = 0: a scene point in the query's face", (0, 0, 0, 0, 0, 0, 0, 0, 0), (-4, -4, 0, 4, -4, 0, 0, 4, 0), 1),
    ("AB = AC = 0: a scene point beside the query", (3, 3, 0, 0, 0, 0, 0, 0, 0), (-4, -4, 0, 4, -4, 0, 0, 4, 0), 0),
    ("zero area on both sides: crossing segments", (-1, 0, 0, 2, 0, 0, 0, 0, 0), (0, -1, 0, 0, 1, 0, 0, 1, 0), 1),
    ("zero area on both sides: the same point", (1, 2, 3, 0, 0, 0, 0, 0, 0), (1, 2, 3) * 3, 1),
    ("zero area on both sides: two points", (1, 2, 3, 0, 0, 0, 0, 0, 0), (1, 2, 3.5) * 3, 0),
]


@pytest.mark.parametrize("name,tri,q,want", TRIANGLE_CASES, ids=[c[0] for c in TRIANGLE_CASES])
def test_exact_triangle_cases(name, tri, q, want):
    for kind in (T.TRIANGLE, T.LIGHT):
        assert overlap(kind, [tri], [q])[0] == want
    assert T.sat23_f64(np.array([tri], f32), np.array([q], f32))[0] == bool(want)  # (the yardstick agrees)
    d = T.distance_f64(np.array([tri], f32), np.array([q], f32))[0]
    if not want:
        assert d > 0  # (apart: a positive distance)


def test_the_named_axes_are_the_only_ones_that_separate():
    """The two cases named after one family of axes: in float64, the family's axes separate and no other does."""
    def separating(tri, q):
        P, Q = T._shapes64(np.array([tri], f32), np.array([q], f32))
        e = [P[1] - P[0], P[2] - P[1], P[0] - P[2]]
        f = [Q[1] - Q[0], Q[2] - Q[1], Q[0] - Q[2]]
        nP, nQ = np.cross(e[0], e[1]), np.cross(f[0], f[1])
        fam = {"normals": [nP, nQ], "hulls": [u[None, :] for u in np.eye(3)], "cross": [np.cross(a, b) for a in e for b in f],
               "in-plane": [np.cross(nP, a) for a in e] + [np.cross(nQ, b) for b in f] + [np.cross(nP, b) for b in f]
               + [np.cross(nQ, a) for a in e]}
        out = set()
        for name, axes in fam.items():
            for a in axes:
                x, y = [(a * p).sum() for p in P], [(a * p).sum() for p in Q]
                if min(x) > max(y) or min(y) > max(x):
                    out.add(name)
        return out
    assert separating(RIGHT, (3, 3, 0, 5, 3, 0, 3, 5, 0)) == {"in-plane"}
    assert separating(SKEW, (0, -3, 4, 0, 4, -3, 1, 3, 3)) == {"cross"}


def test_non_finite_corners_return_zero():
    q = (2, -2, -1, 2, 2, -1, 2, 0, 3)
    assert overlap(T.TRIANGLE, [RIGHT], [q])[0] == 1
    prims = ((T.TRIANGLE, RIGHT), (T.LIGHT, RIGHT), (T.PLANE, (0, 0, 1, 0, 0, 0)), (T.SPHERE, (2, 0, 0, 4)))
    for kind, prim in prims:
        assert overlap(kind, [prim], [q])[0] == 1
    for bad in (NAN, INF, -INF):
        for slot in range(9):  # the query's nine slots, for every kind
            t = list(q)
            t[slot] = bad
            for kind, prim in prims:
                assert overlap(kind, [prim], [t])[0] == 0, (kind, slot, bad)
        for slot in range(9):  # the scene triangle's nine
            tri = list(RIGHT)
            tri[slot] = bad
            assert overlap(T.TRIANGLE, [tri], [q])[0] == 0, (slot, bad)
        for kind, prim in prims[2:]:
            for slot in range(len(prim)):
                p = list(prim)
                p[slot] = bad
                assert overlap(kind, [p], [q])[0] == 0, (kind, slot, bad)
    assert overlap(T.SPHERE, [(2, 0, 0, -1)], [q])[0] == 0  # a negative squared radius
    # corners that overflow in A + AB
    assert overlap(T.TRIANGLE, [(3e38, 0, 0, 3e38, 0, 0, 0, 1, 0)], [(-3e38, -1, -1, 3e38, 1, 1, 0, 0, 0)])[0] == 0


def test_exact_plane_and_sphere_cases():
    plane = (0, 0, 1, 7, -3, 2)  # z = 2
    tris = [(0, 0, 0, 1, 0, 1, 0, 1, 1),    # below
            (0, 0, 1, 1, 0, 1, 0, 1, 2),    # a corner on the plane
            (0, 0, 2, 1, 0, 2, 0, 1, 2),    # in the plane
            (0, 0, 1, 1, 0, 4, 0, 1, 3),    # crossing
            (0, 0, 2, 1, 0, 3, 0, 1, 4),    # above, a corner on the plane
            (0, 0, 2 + 2.0 ** -16, 1, 0, 3, 0, 1, 4),  # above by 2^-16 (the slack at M = 7 is under 2^-17)
            (5, 5, 2) * 3,                  # a point of the plane
            (5, 5, 1) * 3]                  # a point below
    want = [0, 1, 1, 1, 1, 0, 1, 0]
    assert list(overlap(T.PLANE, [plane] * len(tris), tris)) == want
    assert list(T.plane_f64(np.array([plane] * len(tris), f32), np.array(tris, f32))) == [bool(w) for w in want]
    sphere = (1, 1, 1, 4)  # radius 2 about (1, 1, 1)
    tris = [(0.5, 0.5, 0.5, 1.5, 1.5, 0.5, 1.5, 0.5, 1.5),  # wholly inside the sphere: does not touch the surface
            (-5, 1, 1, 5, -4, 1, 5, 6, 1),                  # through the centre, corners outside
            (3, 0, 0, 3, 2, 0, 3, 1, 2),                    # touches from outside (x = 3)
            (3.5, 0, 0, 3.5, 2, 0, 3.5, 1, 2),              # outside
            (1, 1, 1, 3, 1, 1, 1, 2, 1),                    # inside, its farthest corner on the surface
            (1, 1, 1, 2, 2, 2, 1, 2, 1),                    # inside (farthest corner at sqrt(3) < 2)
            (3, 1, 1) * 3,                                  # a point of the surface
            (1, 1, 1) * 3]                                  # the centre
    want = [0, 1, 1, 0, 1, 0, 1, 0]
    assert list(overlap(T.SPHERE, [sphere] * len(tris), tris)) == want
    assert list(T.sphere_f64(np.array([sphere] * len(tris), f32), np.array(tris, f32))) == [bool(w) for w in want]


# ---- the contract ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=T.OFFSETS, ids=["offset%g" % o for o in T.OFFSETS])
def pairs(request):
    import mobileraytracer_amd as m
    off = request.param
    tri, q = T.contract_pairs(1 << 20, 100 + int(off), off)
    got = m.triangle_overlap(T.TRIANGLE, tri, q) != 0
    return off, tri, q, got, T.sat23_f64(tri, q)


def test_the_accepted_share_is_between_5_and_50_percent(pairs):
    off, tri, q, got, exact = pairs
    print("offset %g: float64 accepts %.4f, the function %.4f" % (off, exact.mean(), got.mean()))
    assert 0.05 <= got.mean() <= 0.50


def test_no_intersecting_pair_is_lost(pairs):
    """(a): no pair that float64 finds intersecting on the stored corners and the function rejects."""
    off, tri, q, got, exact = pairs
    lost = exact & ~got
    assert not lost.any(), (int(lost.sum()), tri[lost][0], q[lost][0])


def test_every_acceptance_is_explained_by_a_distance_of_4_g_eps_m(pairs):
    """(b): no pair the function accepts that float64 finds apart by more than 4 g eps M."""
    off, tri, q, got, exact = pairs
    extra = got & ~exact
    d = T.distance_f64(tri[extra], q[extra]) / (T.EPS * T.scale_of(T.TRIANGLE, tri[extra], q[extra]))
    for g in (T.G / 4, T.G / 2, T.G):
        print("offset %g: g = %g leaves %d of %d acceptances unexplained" % (off, g, int((d > g).sum()), int(got.sum())))
    assert not (d > 4 * T.G).any(), (int((d > 4 * T.G).sum()), float(d.max()))


def test_an_accepted_pair_s_hulls_overlap(pairs):
    """The cull's premise: triangle_overlap == 1 implies that the float32 hulls overlap in closed compares."""
    off, tri, q, got, exact = pairs
    assert not (got & ~T.hulls_overlap(tri, q)).any()


FAMILIES = {  # name: (kind, generator, contract (b) claimed)
    "coplanar": (T.TRIANGLE, lambda n: T.coplanar_pairs(n, 5), True),
    "shared corner": (T.TRIANGLE, lambda n: T.shared_pairs(n, 6, 1), True),
    "shared edge": (T.TRIANGLE, lambda n: T.shared_pairs(n, 7, 2), True),
    "query segments": (T.TRIANGLE, lambda n: T.segment_pairs(n, 8), True),
    "query points": (T.TRIANGLE, lambda n: T.point_pairs(n, 9), True),
    "both degenerate": (T.TRIANGLE, lambda n: T.degenerate_pairs(n, 10), False),
    "planes": (T.PLANE, lambda n: T.plane_pairs(n, 11), True),
    "spheres": (T.SPHERE, lambda n: T.sphere_pairs(n, 12), True),
}


@pytest.mark.parametrize("name", list(FAMILIES))
def test_further_families_keep_the_contract(name):
    import mobileraytracer_amd as m
    kind, make, claimed = FAMILIES[name]
    prims, q = make(1 << 16)
    got = m.triangle_overlap(kind, prims, q) != 0
    exact = T.F64[kind](prims, q)
    print("%s: accepted %.4f, float64 %.4f" % (name, got.mean(), exact.mean()))
    if not name.startswith("shared"):  # (the family exercises both answers)
        assert exact.mean() >= 0.03 and not got.all()
    lost = exact & ~got
    assert not lost.any(), (int(lost.sum()), prims[lost][0], q[lost][0])
    if kind == T.TRIANGLE:
        assert not (got & ~T.hulls_overlap(prims, q)).any()
    if claimed:
        M = T.scale_of(kind, prims, q)
        for g in (T.G / 4, T.G / 2, T.G):
            print("%s: g = %g leaves %d unexplained" % (name, g, int((got & ~T.F64[kind](prims, q, g * T.EPS * M)).sum())))
        loose = got & ~T.F64[kind](prims, q, 4 * T.G * T.EPS * M)
        assert not loose.any(), (int(loose.sum()), prims[loose][0], q[loose][0])


def test_a_light_is_a_triangle():
    import mobileraytracer_amd as m
    tri, q = T.contract_pairs(1 << 12, 3, 100.0)
    assert np.array_equal(m.triangle_overlap(T.LIGHT, tri, q), m.triangle_overlap(T.TRIANGLE, tri, q))
    tri, q = T.coplanar_pairs(1 << 12, 4)
    assert np.array_equal(m.triangle_overlap(T.LIGHT, tri, q), m.triangle_overlap(T.TRIANGLE, tri, q))


def test_the_header_s_g_is_the_tests():
    with open(os.path.join(REPO, "mobileraytracer_amd", "csrc", "mrt_triangle_overlap.hpp")) as f:
        assert "constexpr float kTriOverlapG = %.1fF;" % T.G in f.read()


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
    f = dict(a=0x1000, b=0x2000, c=0x3000, aStride=3, bStride=3, cStride=3, n=4)
    f.update(kw)
    return _native.MrtTriangleBatch(**f)


def _outputs(**kw):
    """All five fields set (the pointers stand for device memory: never dereferenced here)."""
    from mobileraytracer_amd import _native
    f = {name: 0x10000 * (k + 1) for k, name in enumerate(FIELDS)}
    f.update(kw)
    return _native.MrtOverlaps(**f)


def _call(lib, handle, batch, out, k=4, size=None):
    size = ctypes.sizeof(out) if size is None and out is not None else (size or 0)
    rc = lib.mrt_overlap_triangles_device(handle, None if batch is None else ctypes.byref(batch), k,
                                          None if out is None else ctypes.byref(out), size, None)
    return rc, lib.mrt_last_error()


def test_rejects_null_arguments(lib, fake):
    rc, msg = _call(lib, None, _batch(), _outputs())
    assert rc == -1 and b"mrt_overlap_triangles_device" in msg and b"null renderer" in msg
    rc, msg = _call(lib, fake, None, _outputs())
    assert rc == -1 and b"mrt_overlap_triangles_device" in msg and b"null triangle batch" in msg
    rc, msg = _call(lib, fake, _batch(), None, size=40)
    assert rc == -1 and b"null outputs" in msg
    for kw in ({"a": None}, {"b": None}, {"c": None}):
        rc, msg = _call(lib, fake, _batch(**kw), _outputs())
        assert rc == -1 and b"null a / b / c" in msg
    # ... each of them with a NULL handle too: the handle is checked first and never read
    for batch, out, k in ((None, _outputs(), 4), (_batch(c=None), _outputs(), 4), (_batch(n=0), _outputs(), 4),
                          (_batch(), _outputs(), 0)):
        rc, msg = _call(lib, None, batch, out, k=k)
        assert rc == -1 and b"null renderer" in msg


@pytest.mark.parametrize("k", [0, -1, 17, 1 << 20, -(1 << 31)])
def test_rejects_a_k_outside_one_to_sixteen(lib, fake, k):
    rc, msg = _call(lib, fake, _batch(), _outputs(), k=k)
    assert rc == -1 and b"mrt_overlap_triangles_device" in msg and b"K must be 1 .. 16" in msg


@pytest.mark.parametrize("size", [0, 1, 7])
def test_rejects_a_size_that_cannot_hold_any(lib, fake, size):
    out = _outputs()
    rc = lib.mrt_overlap_triangles_device(fake, ctypes.byref(_batch()), 4, ctypes.byref(out), size, None)
    assert rc == -1 and b"outSize" in lib.mrt_last_error() and b"any" in lib.mrt_last_error()


def test_rejects_no_wanted_output_and_cuts_fields_at_the_size(lib, fake):
    rc, msg = _call(lib, fake, _batch(), _outputs(**{name: None for name in FIELDS}))
    assert rc == -1 and b"no output" in msg
    # fields beyond outSize count as null: only any, count, kind are within 24 bytes
    rc, msg = _call(lib, fake, _batch(), _outputs(any=None, count=None, kind=None), size=24)
    assert rc == -1 and b"no output" in msg
    # ... and a field cut in half is not within it
    rc, msg = _call(lib, fake, _batch(), _outputs(any=None, count=None, kind=None), size=31)
    assert rc == -1 and b"no output" in msg
    rc, msg = _call(lib, fake, _batch(), _outputs(any=None), size=8)
    assert rc == -1 and b"no output" in msg


@pytest.mark.parametrize("n", [0, -1, 1 << 31, -(1 << 31), 1 << 40])
def test_rejects_a_triangle_count_outside_the_int_range(lib, fake, n):
    rc, msg = _call(lib, fake, _batch(n=n), _outputs())
    assert rc == -1 and b"n must be" in msg


@pytest.mark.parametrize("stride", [1, 2, -1, -(1 << 40)])
def test_rejects_a_stride_below_three(lib, fake, stride):
    for kw in ({"aStride": stride}, {"bStride": stride}, {"cStride": stride}):
        rc, msg = _call(lib, fake, _batch(**kw), _outputs())
        assert rc == -1 and b"mrt_overlap_triangles_device" in msg and b"stride" in msg


def test_triangle_overlap_checks_its_arguments(lib):
    ptr = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    for kind in (0, 5, -1):
        assert lib.mrt_triangle_overlap(kind, ptr, ptr, 1, ptr) == -1 and b"kind" in lib.mrt_last_error()
    assert lib.mrt_triangle_overlap(3, None, ptr, 1, ptr) == -1 and b"null" in lib.mrt_last_error()
    assert b"mrt_triangle_overlap" in lib.mrt_last_error()
    assert lib.mrt_triangle_overlap(3, ptr, None, 1, ptr) == -1
    assert lib.mrt_triangle_overlap(3, ptr, ptr, 1, None) == -1
    assert lib.mrt_triangle_overlap(3, ptr, ptr, -1, ptr) == -1
    assert lib.mrt_triangle_overlap(3, ptr, ptr, 0, ptr) == 0


def test_the_wrapper_takes_both_shapes_and_checks_the_counts():
    import mobileraytracer_amd as m
    tri, q = T.contract_pairs(64, 1, 0.0)
    flat = m.triangle_overlap(T.TRIANGLE, tri, q)
    assert flat.dtype == np.int32 and flat.shape == (64,)
    assert np.array_equal(m.triangle_overlap(T.TRIANGLE, tri, q.reshape(64, 3, 3)), flat)
    with pytest.raises(ValueError):
        m.triangle_overlap(T.TRIANGLE, tri, q[:63])


def test_structs_match_the_header(tmp_path):
    """ctypes MrtTriangleBatch has the size and the field offsets of the C structure, the outputs are
    mrt_overlaps, and the symbols are exported."""
    from mobileraytracer_amd import _native
    batch = ("a", "b", "c", "aStride", "bStride", "cStride", "n")
    assert [f for f, _ in _native.MrtTriangleBatch._fields_] == list(batch)
    src = tmp_path / "triangles.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mobilert_amd.h"\n'
                   'int main(void){printf("%d %zu %zu", MRT_OVERLAP_MAX, sizeof(mrt_overlaps), sizeof(mrt_triangle_batch));'
                   + "".join('printf(" %%zu", offsetof(mrt_triangle_batch, %s));' % f for f in batch) + 'return 0;}')
    exe = tmp_path / "triangles"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [_native.OVERLAP_MAX, ctypes.sizeof(_native.MrtOverlaps), ctypes.sizeof(_native.MrtTriangleBatch)] + [
        getattr(_native.MrtTriangleBatch, f).offset for f in batch]
    assert got == [16, 40, 56] + [8 * k for k in range(7)]
    for name in ("mrt_overlap_triangles_device", "mrt_triangle_overlap", "mrt_kat_triangle_overlap"):
        assert name in _native.EXPORTED_SYMBOLS
