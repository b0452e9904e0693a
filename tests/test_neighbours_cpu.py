"""Neighbour queries without a device: the argument errors of mrt_neighbours_device, all checked before the
renderer is read; the ctypes structure against the header; and the test helper (neighbour_cases.Lists)
against the nearest-point helper it must agree with at K = 1."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import nearest_cases as N
import neighbour_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_BYTES = 1 << 16
FILL = b"\xa5"
FIELDS = ("count", "kind", "index", "dist2", "point", "bary", "tests")
f32 = np.float32


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
    """All seven fields set (the pointers stand for device memory: never dereferenced here)."""
    from mobileraytracer_amd import _native
    f = {name: 0x10000 * (k + 1) for k, name in enumerate(FIELDS)}
    f.update(kw)
    return _native.MrtNeighbours(**f)


def _call(lib, handle, batch, out, k=4, size=None):
    size = ctypes.sizeof(out) if size is None and out is not None else (size or 0)
    rc = lib.mrt_neighbours_device(handle, None if batch is None else ctypes.byref(batch), k,
                                   None if out is None else ctypes.byref(out), size, None)
    return rc, lib.mrt_last_error()


def test_rejects_null_arguments(lib, fake):
    rc, msg = _call(lib, None, _batch(), _outputs())
    assert rc == -1 and b"mrt_neighbours_device" in msg and b"null renderer" in msg
    rc, msg = _call(lib, fake, None, _outputs())
    assert rc == -1 and b"null point batch" in msg
    rc, msg = _call(lib, fake, _batch(), None, size=56)
    assert rc == -1 and b"null outputs" in msg
    rc, msg = _call(lib, fake, _batch(point=None), _outputs())
    assert rc == -1 and b"null point" in msg
    # ... each of them with a NULL handle too: the handle is checked first and never read
    for batch, out, k in ((None, _outputs(), 4), (_batch(point=None), _outputs(), 4), (_batch(n=0), _outputs(), 4),
                          (_batch(), _outputs(), 0)):
        rc, msg = _call(lib, None, batch, out, k=k)
        assert rc == -1 and b"null renderer" in msg


@pytest.mark.parametrize("k", [0, -1, 17, 1 << 20, -(1 << 31)])
def test_rejects_a_k_outside_one_to_sixteen(lib, fake, k):
    rc, msg = _call(lib, fake, _batch(), _outputs(), k=k)
    assert rc == -1 and b"K must be 1 .. 16" in msg


@pytest.mark.parametrize("size", [0, 1, 7])
def test_rejects_a_size_that_cannot_hold_count(lib, fake, size):
    out = _outputs()
    rc = lib.mrt_neighbours_device(fake, ctypes.byref(_batch()), 4, ctypes.byref(out), size, None)
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
def test_rejects_a_point_count_outside_the_int_range(lib, fake, n):
    rc, msg = _call(lib, fake, _batch(n=n), _outputs())
    assert rc == -1 and b"n must be" in msg


@pytest.mark.parametrize("stride", [1, 2, -1, -(1 << 40)])
def test_rejects_a_stride_below_three(lib, fake, stride):
    rc, msg = _call(lib, fake, _batch(stride=stride), _outputs())
    assert rc == -1 and b"stride" in msg


def test_struct_matches_the_header(tmp_path):
    """ctypes MrtNeighbours has the size and the field offsets of the C structure, MRT_NEIGHBOURS_MAX is the
    wrapper's limit, and the symbol is exported."""
    from mobileraytracer_amd import _native
    assert [f for f, _ in _native.MrtNeighbours._fields_] == list(FIELDS)
    assert [name for name, _, _ in _native.NEIGHBOUR_FIELDS] == list(FIELDS)
    assert {name: w for name, _, w in _native.NEIGHBOUR_FIELDS} == C.WIDTHS
    src = tmp_path / "neighbours.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mobilert_amd.h"\n'
                   'int main(void){printf("%d %zu", MRT_NEIGHBOURS_MAX, sizeof(mrt_neighbours));'
                   + "".join('printf(" %%zu", offsetof(mrt_neighbours, %s));' % f for f in FIELDS) + 'return 0;}')
    exe = tmp_path / "neighbours"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [_native.NEIGHBOURS_MAX, ctypes.sizeof(_native.MrtNeighbours)] + [
        getattr(_native.MrtNeighbours, f).offset for f in FIELDS]
    assert got == [16, 56] + [8 * k for k in range(7)]
    assert C.K_MAX == _native.NEIGHBOURS_MAX
    assert "mrt_neighbours_device" in _native.EXPORTED_SYMBOLS


def test_the_helper_at_k_1_is_the_nearest_point_helper(tmp_path):
    """On 256 points of the 300-triangle soup - in its box, near its surface, on its corners - with and
    without radii and sources, the K = 1 list equals nearest_cases.Candidates.expected in every field, and
    the lists for larger K are sorted, start with it and hold count entries."""
    import mobileraytracer_amd as m
    cfg = C.obj_cfg(C.soup(str(tmp_path), "soup", 0.0, 0.2))
    geom = m.scene_triangles(cfg)[0]
    assert len(geom) == 300
    pts = C.soup_points(geom, 86, 1e-3)[:256]
    lists = C.Lists(cfg)
    assert len(lists.kind) == 302 and lists.fixed == 2
    d2 = lists.distances(pts)
    rng = np.random.default_rng(5)
    radius = rng.choice([0.05, 0.2, 1.0, 0.0, -1.0, np.nan], 256).astype(f32)
    src = np.stack([np.full(256, N.TRIANGLE), np.argmin(d2[:, :300], 1)], 1).astype(np.int32)  # (the nearest triangle)
    for kw in ({}, {"max_dist": radius}, {"src": src}, {"max_dist": radius, "src": src}):
        one = lists.expected(pts, 1, d2=d2, **kw)
        ref = lists.cands.expected(pts, **kw)
        N.assert_same({f: one[f][:, 0] for f in N.FIELDS}, ref, "K = 1, %s" % sorted(kw))
        assert np.array_equal(one["count"] > 0, ref["kind"] > 0)
        many = lists.expected(pts, 16, d2=d2, **kw)
        C.assert_same(C.cut(many, 1), one, "the first of 16, %s" % sorted(kw))
        assert np.array_equal(many["count"], one["count"])
        held = np.arange(16)[None, :] < many["count"][:, None]
        assert np.array_equal(many["kind"] > 0, held) and np.array_equal(many["index"] >= 0, held)
        assert (many["dist2"][:, 1:] >= many["dist2"][:, :-1]).all()  # (ascending, then the bound as padding)
        b2 = C.bound2_of(256, kw.get("max_dist"))
        assert np.array_equal(C.bits(many["dist2"][~held]), C.bits(np.broadcast_to(b2[:, None], held.shape)[~held]))
        assert (many["point"][~held] == 0).all() and (many["bary"][~held] == 0).all()
        if "src" in kw:
            assert not ((many["kind"] == N.TRIANGLE) & (many["index"] == src[:, 1:])).any()
    assert (lists.expected(pts, 16, d2=d2)["count"] == 302).all()
