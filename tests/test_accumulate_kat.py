"""Known-answer test of the float -> pixel conversion and the running average (incrementalAvg,
Utils.cpp:66-90) as the accumulation kernels compute them.

The reference's ``static_cast<uint32_t>(sample * 255)`` is, on its x86-64 build, a 64-bit truncation
of which the low 32 bits are kept: negative radiance wraps, and NaN, +-inf and everything from 2^63
on give 0.  The GPU's own conversion saturates, so the kernels restate the rule (x86TruncU32,
DESIGN.md section 4).

* CPU half: the oracle's ``incremental_avg`` against a numpy restatement of that definition, so the
  oracle is pinned by a definition and not by one compiler's code generation.
* GPU half: ``mrt_kat_accumulate`` runs k_accumulate (mode 0) and k_resolve_accumulate (mode 1, every
  vertex terminal) on a table of such values, bit-exact against the oracle folded in sample order.
"""
import functools

import numpy as np
import pytest

F = np.float32
W, H, N_SLOTS = 64, 32, 1000  # 1000 of the frame's 2048 slots: the last block and wave are partial
SENTINEL = np.int32(0x12345678)  # alpha 0x12: never produced by incrementalAvg (alpha 0xFF)


def around(x):
    """x as float32 and its two float32 neighbours."""
    x = F(x)
    return [np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))]


def value_table():
    v = [F(0.0), F(1e-40), F(-0.0)]
    for k in (1, 127, 128, 254, 255):
        v += around(F(k) / F(255))
    v += [F(1.0), F(1.5), F(1e10)]
    v += around(F(2.0 ** 32) / F(255))
    v += [F(2.0 ** 40) / F(255), F(2.0 ** 62) / F(255), F(2.0 ** 63) / F(255), F(2.0 ** 64) / F(255), F(1e20), F(3.4e38)]
    v += [F(np.inf), F(-np.inf), F(np.nan)]
    v += [F(-1e-3)] + around(F(-1) / F(255)) + [F(-3) / F(255), F(-1.0), F(-1e10), F(-1e20)]
    return np.array(v, F)


TABLE = value_table()


# ---- the definition, in numpy ---------------------------------------------------------------------
def trunc_u32(x):
    """float32 radiance -> the channel's uint32: f = float32(x) * float32(255); the low 32 bits of
    trunc(f) as a 64-bit integer where |f| < 2^63, and 0 otherwise (NaN included)."""
    with np.errstate(all="ignore"):
        f = np.asarray(x, F) * F(255)
        assert f.dtype == F
        ok = np.abs(f) < F(2.0 ** 63)  # False for NaN
        t = np.trunc(np.where(ok, f, F(0)).astype(np.float64))  # exact: a float32 is a float64
    return (t.astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def incremental_avg_np(rgb, avg, n):
    """incrementalAvg on arrays: rgb (..., 3) float32, avg int32 bits, n >= 1; uint32 arithmetic."""
    a = np.asarray(avg).astype(np.int64) & 0xFFFFFFFF
    s = trunc_u32(rgb).astype(np.int64)
    n = np.asarray(n, np.int64)
    out = np.full(a.shape, 0xFF000000, np.int64)
    for c in range(3):
        last = (a >> (8 * c)) & 0xFF
        cur = (((n - 1) * last + s[..., c]) & 0xFFFFFFFF) // n
        out |= np.minimum(cur, 255) << (8 * c)
    return out.astype(np.uint32).view(np.int32)


def u32(v):
    return int(v) & 0xFFFFFFFF


# ---- CPU half ---------------------------------------------------------------------------------------
def test_table_reaches_every_range():
    """The table has what it is there for: both sides of 2^32 and of 2^63, the wrap, the non-finite."""
    with np.errstate(all="ignore"):
        f = TABLE * F(255)
    assert (f == F(2.0 ** 32)).any() and (f == np.nextafter(F(2.0 ** 32), F(0))).any() and (f > F(2.0 ** 32)).any()
    assert (f == F(2.0 ** 62)).any() and (f == F(2.0 ** 63)).any() and (f == F(2.0 ** 64)).any()
    # (3.4e38 * 255 overflows: a finite radiance whose product is +inf)
    assert np.isnan(f).sum() == 1 and np.isposinf(f).sum() == 2 and np.isneginf(f).sum() == 1
    assert (f == F(-1.0)).any() and (f == F(-3.0)).any() and ((f < 0) & (f > -1)).any() and (f < F(-2.0 ** 63)).any()
    assert np.signbit(TABLE[2]) and TABLE[2] == 0 and 0 < TABLE[1] < np.finfo(F).tiny


def test_oracle_rows_quoted_in_the_design(oracle_mod):
    """One sample (avg 0, n 1), the value in all three channels."""
    inc = oracle_mod.incremental_avg
    rows = [
        (np.inf, 0xFF000000), (-np.inf, 0xFF000000), (np.nan, 0xFF000000),
        (1e20, 0xFF000000), (-1e20, 0xFF000000),
        (F(2.0 ** 32) / F(255), 0xFF000000),  # f * 255 = 2^32 exactly: the low word is 0
        (1e10, 0xFFFFFFFF), (-1e10, 0xFFFFFFFF),
        (F(-1) / F(255), 0xFFFFFFFF), (F(-3) / F(255), 0xFFFFFFFF), (-1.0, 0xFFFFFFFF),  # wraps
        (-0.001, 0xFF000000),
    ]
    assert F(F(2.0 ** 32) / F(255)) * F(255) == F(2.0 ** 32)
    for x, want in rows:
        x = float(F(x))
        assert u32(inc((x, x, x), 0, 1)) == want, (x, hex(u32(inc((x, x, x), 0, 1))))
        assert u32(incremental_avg_np(np.array([x, x, x], F), 0, 1)) == want, x
    # the wrapped uint32 arithmetic goes on: (2 * 128 + (2^32 - 3)) mod 2^32 = 253, / 3 = 84
    x = float(F(-3) / F(255))
    assert u32(inc((x, x, x), 0x00808080, 3)) == 0xFF545454
    assert u32(incremental_avg_np(np.array([x, x, x], F), 0x00808080, 3)) == 0xFF545454


def test_oracle_conversion_matches_the_definition(oracle_mod):
    """Every table value in each channel (the other two ordinary), over a set of running averages and
    sample numbers: the oracle equals the numpy restatement of the definition."""
    rng = np.random.default_rng(11)
    prior = [0, 0x00808080, u32(-1)] + [int(x) for x in rng.integers(0, 1 << 32, 5)]
    for c in range(3):
        for x in TABLE:
            rgb = rng.random(3).astype(F)
            rgb[c] = x
            for avg in prior:
                avg32 = int(np.uint32(avg).view(np.int32))
                for n in (1, 2, 3, 8, 256):
                    got = oracle_mod.incremental_avg([float(v) for v in rgb], avg32, n)
                    want = incremental_avg_np(rgb, avg32, n)
                    assert u32(got) == u32(want), (c, x, hex(avg), n, hex(u32(got)), hex(u32(want)))


# ---- GPU half ---------------------------------------------------------------------------------------
def records(spp):
    """N_SLOTS * spp radiance records: record (slot, s) carries table entry (slot + 37 s) mod (3 T)
    - a value and the channel it sits in; the other two channels ordinary - so every (value,
    channel) is met at every sample position.  Every 11th record is ordinary in all three."""
    rng = np.random.default_rng(1000 + spp)
    rgb = rng.random((N_SLOTS, spp, 3)).astype(F)
    slot, s = np.meshgrid(np.arange(N_SLOTS), np.arange(spp), indexing="ij")
    combo = (slot + 37 * s) % (3 * len(TABLE))
    special = (slot * spp + s) % 11 != 0
    ch = combo // len(TABLE)
    for c in range(3):
        m = special & (ch == c)
        rgb[m, c] = TABLE[combo[m] % len(TABLE)]
    return rgb


@functools.lru_cache(maxsize=None)
def case(spp, sample_base, oracle_mod):
    """(records, prior bitmap, expected bitmap): the oracle's incremental_avg folded in sample order
    over each slot's records, from the prior pixel (sample_base > 0) or 0; other pixels untouched."""
    from mobileraytracer_amd import sharding
    rgb = records(spp)
    pix = sharding.slot_pixels(W, H, 0, 1)
    assert len(pix) == W * H and len(set(pix.tolist())) == W * H
    rng = np.random.default_rng(7 * spp + sample_base)
    if sample_base > 0:
        prior = (rng.integers(0, 1 << 24, W * H).astype(np.uint32) | np.uint32(0xFF000000)).view(np.int32)
    else:
        prior = np.full(W * H, SENTINEL, np.int32)
    want = prior.copy()
    for q in range(N_SLOTS):
        c = int(prior[pix[q]]) if sample_base > 0 else 0
        for s in range(spp):
            c = oracle_mod.incremental_avg(rgb[q, s].tolist(), c, sample_base + s + 1)
        want[pix[q]] = c
    for a in (rgb, prior, want):
        a.setflags(write=False)
    return rgb, prior, want


@pytest.mark.gpu
@pytest.mark.parametrize("sample_base", [0, 1, 7, 255])
@pytest.mark.parametrize("spp", [1, 3, 4, 5, 16, 64, 128])
def test_accumulation_kernels_match_the_oracle(oracle_mod, spp, sample_base):
    import mobileraytracer_amd as m
    rgb, prior, want = case(spp, sample_base, oracle_mod)
    for mode in (0, 1):
        bm = prior.copy()
        launched = m.kat_accumulate(rgb.reshape(-1, 3), spp, sample_base, bm, W, H, mode)
        if mode == 1 and 64 % spp != 0:  # a slot's samples would not share a wave: refused
            assert not launched and np.array_equal(bm, prior)
            continue
        assert launched
        bad = np.flatnonzero(bm != want)
        print("spp %d base %d mode %d: %d of %d pixels differ" % (spp, sample_base, mode, len(bad), W * H))
        assert len(bad) == 0, [(int(p), hex(u32(bm[p])), hex(u32(want[p]))) for p in bad[:8]]
