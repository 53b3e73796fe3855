"""minhash on the MI355X, bit for bit against the model of tests/minhash_model.py (checked against minhash_ops.h by
tests/test_minhash_cpu.py), through the C ABI and through custrings_amd/minhash.py: the wave and workgroup edges of the row
count, permutation counts with a ragged last chunk and on either side of the LDS result block, both forms with the route
asserted, null rows at the ends of a tile, rows shorter than an n-gram, long rows (an n-gram count on either side of a
segment, a last character of four bytes, continuation bytes only), a borrowed column at an odd address, results to host and
to device memory with the words beside them watched, the band keys and their way into nvcategory.from_numbers, the estimate
against a known Jaccard similarity, and every argument error."""
import ctypes as C
import math

import numpy as np
import pytest

import borrowedutil as bu
import gpuutil
import minhash_model as m
from test_minhash_cpu import A4, B4, EXAMPLE

pytestmark = pytest.mark.gpu

WIDTH, SEED = 5, 3


def _L():
    return gpuutil.lib()


def _route():
    return _L().lib.cs_debug_last_route().decode()


def column(rows):
    from custrings_amd import nvstrings

    _L()
    chars, offs, nulls = m.to_arrow(rows)
    valid = np.concatenate([np.packbits(1 - nulls, bitorder="little"), np.zeros(8, dtype=np.uint8)])
    chars = chars if chars.size else np.zeros(1, dtype=np.uint8)
    return nvstrings.from_offsets64(chars, offs, len(rows), valid)


def perms(nperm, seed=SEED):
    from custrings_amd import minhash

    return minhash.permutations(nperm, seed)


def abi_minhash(g, width, seed, a, b, rows, guard=4):
    """cs_minhash into host memory with `guard` canary words on either side -> rows x nperm"""
    L = _L()
    n = len(a)
    buf = np.full(rows * n + 2 * guard, 0xA5A5A5A5, dtype=np.uint32)
    L.check(L.lib.cs_minhash(g.m_cptr, width, seed, a.ctypes.data, b.ctypes.data, n, buf[guard:].ctypes.data, 0, None))
    assert np.all(buf[:guard] == 0xA5A5A5A5) and np.all(buf[guard + rows * n:] == 0xA5A5A5A5), "words beside the results were written"
    return buf[guard:guard + rows * n].reshape(rows, n)


def with_nulls_at_tile_ends(rows):
    rows = list(rows)
    for at in (0, 31, 63, 64, len(rows) - 1):
        if at < len(rows):
            rows[at] = None
    return rows


_want = {}


def short_case(nrows, nperm):
    """the rows of a short-form case and the model's signatures, computed once"""
    key = (nrows, nperm)
    if key not in _want:
        rows = m.mixed_rows(nrows, 100 + nrows)
        if nrows >= 63:
            rows = with_nulls_at_tile_ends(rows)
        a, b = perms(nperm)
        _want[key] = (rows, a, b, m.signatures(rows, WIDTH, SEED, a, b))
    return _want[key]


# ---- the worked example ---------------------------------------------------------------------------------------------------------
def test_worked_example_through_the_module():
    from custrings_amd import minhash, nvstrings

    s = nvstrings.to_device([t for t, _ in EXAMPLE] + [None])
    sig = minhash.minhash(s, width=4, seed=0, a=np.array(A4, dtype=np.uint32), b=np.array(B4, dtype=np.uint32))
    assert sig.dtype == np.uint32 and sig.shape == (6, 4)
    for got, (_, want) in zip(sig, EXAMPLE):
        assert " ".join("%08x" % v for v in got) == want
    assert sig[5].tolist() == [m.NO_GRAM] * 4
    default = minhash.minhash(s)
    a, b = minhash.permutations(128, 0)
    assert default.shape == (6, 128) and np.array_equal(default, m.signatures([t.encode() for t, _ in EXAMPLE] + [None], 5, 0, a, b))


# ---- the short form ---------------------------------------------------------------------------------------------------------------
# (rows, nperm): the wave and workgroup edges; nperm 1 / 7 / 64 fit the LDS result block of a 64-row tile, 65 does not by one
# value a row, 300 fits no tile's; 7, 65 and 300 leave a ragged last chunk
@pytest.mark.parametrize("nrows,nperm", [(1, 1), (63, 7), (64, 65), (65, 300), (257, 64), (257, 7)])
def test_short_rows_take_the_tile_form(nrows, nperm):
    rows, a, b, want = short_case(nrows, nperm)
    got = abi_minhash(column(rows), WIDTH, SEED, a, b, nrows)
    assert _route() == "tile", _route()
    assert np.array_equal(got, want)


def test_rows_shorter_than_an_ngram_and_every_boundary():
    rows = m.boundary_rows(WIDTH) + m.malformed_rows()
    a, b = perms(7)
    got = abi_minhash(column(rows), WIDTH, SEED, a, b, len(rows))
    assert _route() == "tile", _route()
    assert np.array_equal(got, m.signatures(rows, WIDTH, SEED, a, b))


@pytest.mark.parametrize("width", [1, 4, 255])
def test_other_widths(width):
    rows = m.mixed_rows(70, 5) + [m.text_row(n, n) for n in (254, 255, 256, 300)]
    a, b = perms(3)
    got = abi_minhash(column(rows), width, SEED, a, b, len(rows))
    assert _route() == "tile", _route()
    assert np.array_equal(got, m.signatures(rows, width, SEED, a, b))


def test_no_rows_and_no_results_write_nothing():
    from custrings_amd import minhash

    L = _L()
    a, b = perms(4)
    empty = column([])
    assert minhash.minhash(empty, nperm=4).shape == (0, 4)
    buf = np.full(8, 7, dtype=np.uint32)
    assert L.lib.cs_minhash(empty.m_cptr, 5, 0, a.ctypes.data, b.ctypes.data, 4, buf.ctypes.data, 0, None) == 0
    assert L.lib.cs_minhash(column([b"abc"]).m_cptr, 5, 0, a.ctypes.data, b.ctypes.data, 4, None, 0, None) == 0
    assert np.all(buf == 7)
    assert L.lib.cs_minhash_bands(None, 0, 4, 2, buf.ctypes.data, 0, None) == 0 and np.all(buf == 7)


# ---- the long form ------------------------------------------------------------------------------------------------------------------
GRAM_COUNTS = [1, 63, 64, 65, 129, 3000]


def long_rows():
    rows = [m.text_row(c + WIDTH - 1, 40 + c) for c in GRAM_COUNTS]
    rows += [b"ab", None, b"", b"\x80" * 700]  # one n-gram (shorter than it); none; none; 700 bytes and no character: none
    rows += [m.text_row(900, 8, wide_every=0) + "😀".encode()]  # a last character of four bytes
    rows += m.mixed_rows(200, 9)
    rows.insert(100, m.text_row(9000, 10))  # > 10 KB among short rows: no tile size fits this column
    return rows


@pytest.fixture(scope="module")
def long_case():
    rows = long_rows()
    a, b = perms(65)
    return rows, a, b, m.signatures(rows, WIDTH, SEED, a, b)


def test_long_rows_take_the_wave_form(long_case):
    rows, a, b, want = long_case
    assert len(rows[100]) > 10000 and [len(m.ngrams(r, WIDTH)) for r in rows[:6]] == GRAM_COUNTS
    assert want[9].tolist() == [m.NO_GRAM] * 65  # (the model: bytes but no character is no n-gram)
    got = abi_minhash(column(rows), WIDTH, SEED, a, b, len(rows))
    assert _route() == "wave", _route()
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert bad.size == 0, bad.tolist()


@pytest.mark.parametrize("nrows,nperm", [(63, 7), (257, 64)])
def test_wave_form_on_short_rows_gives_the_same(nrows, nperm):
    rows, a, b, want = short_case(nrows, nperm)
    L = _L()
    L.lib.cs_config_set(b"CS_MINHASH_WAVE", b"1")
    try:
        got = abi_minhash(column(rows), WIDTH, SEED, a, b, nrows)
        assert _route() == "wave", _route()
    finally:
        L.lib.cs_config_set(b"CS_MINHASH_WAVE", None)
    assert np.array_equal(got, want)


# ---- borrowed column, device output ----------------------------------------------------------------------------------------------------
def test_borrowed_column_at_an_odd_address_into_a_device_tensor():
    import torch

    from custrings_amd import minhash

    rows, a, b, want = short_case(257, 7)
    _L()
    col = bu.Borrowed(rows, 13, 8, b"\xff")
    out = bu.Guarded(np.uint32, 257 * 7)
    assert minhash.minhash(col.col, width=WIDTH, seed=SEED, a=a, b=b, devptr=out.ptr) == out.ptr
    assert _route() == "tile", _route()
    assert np.array_equal(out.values().reshape(257, 7), want)
    assert col.caller_memory_intact()
    t = torch.zeros((257, 7), dtype=torch.int32, device="cuda:0")
    assert minhash.minhash(col.col, width=WIDTH, seed=SEED, a=a, b=b, devptr=t) is t
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want)


def test_long_rows_into_a_device_buffer(long_case):
    from custrings_amd import minhash

    rows, a, b, want = long_case
    out = bu.Guarded(np.uint32, len(rows) * 65)
    minhash.minhash(column(rows), width=WIDTH, seed=SEED, a=a, b=b, devptr=out.ptr)
    assert _route() == "wave", _route()
    assert np.array_equal(out.values().reshape(len(rows), 65), want)


# ---- band keys ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nperm,bands", [(8, 8), (8, 1), (300, 20)])
def test_band_keys_match_the_model(nperm, bands):
    from custrings_amd import minhash

    rng = np.random.default_rng(nperm + bands)
    sig = rng.integers(0, 1 << 32, size=(67, nperm), dtype=np.uint64).astype(np.uint32)
    sig[5] = m.NO_GRAM
    want = m.band_keys(sig, bands)
    got = minhash.band_keys(sig, bands)
    assert got.dtype == np.int64 and got.shape == (67, bands) and np.array_equal(got, want)
    assert np.array_equal(got >> 32, np.tile(np.arange(bands), (67, 1)))
    import torch

    dsig = torch.from_numpy(sig.view(np.int32)).to("cuda:0")
    out = bu.Guarded(np.int64, 67 * bands)
    minhash.band_keys(dsig, bands, devptr=out.ptr)
    assert np.array_equal(out.values().reshape(67, bands), want)


def test_rows_that_agree_on_one_band_share_exactly_that_key_and_land_under_one_category_key():
    from custrings_amd import minhash, nvcategory

    rng = np.random.default_rng(2)
    sig = rng.integers(0, 1 << 32, size=(6, 12), dtype=np.uint64).astype(np.uint32)
    sig[4, 3:6] = sig[1, 3:6]  # rows 1 and 4 agree on band 1 of 4
    sig[5, 9:12] = sig[0, 9:12]  # rows 0 and 5 on band 3
    keys = minhash.band_keys(sig, 4)
    assert np.array_equal(keys, m.band_keys(sig, 4))
    assert (keys[1] == keys[4]).tolist() == [False, True, False, False] and (keys[0] == keys[5]).tolist() == [False, False, False, True]
    cat = nvcategory.from_numbers(keys.reshape(-1))
    values = np.array(cat.values()).reshape(6, 4)
    pairs = {(i, j) for i in range(6) for j in range(i + 1, 6) if set(values[i].tolist()) & set(values[j].tolist())}
    assert pairs == {(1, 4), (0, 5)}
    assert values[1, 1] == values[4, 1] and values[0, 3] == values[5, 3] and cat.keys_size() == 22


# ---- the estimate ----------------------------------------------------------------------------------------------------------------------------
def test_the_estimate_is_within_four_sigma_of_the_true_jaccard():
    """Two 2 KB rows that share their first 1400 characters.  The bound is the estimator's (4 standard deviations of a mean of
    1024 Bernoulli(J) draws: 0.0623 here); the seed is one for which the MODEL's estimate is inside it: 0.5469 against
    J = 0.5376 at seed 0."""
    from custrings_amd import minhash

    base = m.text_row(2000, 21)
    chars = base.decode()
    other = (chars[:1400] + m.text_row(600, 22).decode()).encode()
    rows = [base, other]
    J = m.jaccard(base, other, 5)
    assert 0.3 < J < 0.9
    bound = 4 * math.sqrt(J * (1 - J) / 1024)
    a, b = minhash.permutations(1024, 0)
    model_sig = m.signatures(rows, 5, 0, a, b)
    assert abs(minhash.jaccard_estimate(model_sig, 0, 1) - J) <= bound
    sig = minhash.minhash(column(rows), width=5, seed=0, nperm=1024)
    print("J %.4f estimate %.4f bound %.4f" % (J, minhash.jaccard_estimate(sig, 0, 1), bound))
    assert np.array_equal(sig, model_sig)
    assert abs(minhash.jaccard_estimate(sig, 0, 1) - J) <= bound


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    L = _L()
    g = column([b"abcdef"])
    a, b = perms(8)
    out = np.zeros(8, dtype=np.uint32)
    keys = np.zeros(8, dtype=np.int64)
    pa, pb, po, pk = a.ctypes.data, b.ctypes.data, out.ctypes.data, keys.ctypes.data
    INVALID, RANGE = L.CS_ERR_INVALID_ARG, L.CS_ERR_RANGE
    mh, bands = L.lib.cs_minhash, L.lib.cs_minhash_bands
    assert mh(None, 5, 0, pa, pb, 8, po, 0, None) == INVALID
    assert mh(g.m_cptr, 5, 0, None, pb, 8, po, 0, None) == INVALID
    assert mh(g.m_cptr, 5, 0, pa, None, 8, po, 0, None) == INVALID
    assert mh(g.m_cptr, 0, 0, pa, pb, 8, po, 0, None) == INVALID
    assert mh(g.m_cptr, 5, 0, pa, pb, 0, po, 0, None) == INVALID
    assert mh(g.m_cptr, 256, 0, pa, pb, 8, po, 0, None) == RANGE
    big = np.ones(4097, dtype=np.uint32)
    assert mh(g.m_cptr, 5, 0, big.ctypes.data, big.ctypes.data, 4097, None, 0, None) == RANGE
    zero = a.copy()
    zero[7] = 0
    assert mh(g.m_cptr, 5, 0, zero.ctypes.data, pb, 8, po, 0, None) == RANGE
    assert "multiplier" in L.last_error()
    assert mh(g.m_cptr, 255, 0, big.ctypes.data, big.ctypes.data, 4096, None, 0, None) == 0  # (the limits themselves are fine)
    assert bands(po, 1, 8, 0, pk, 0, None) == INVALID
    assert bands(po, 1, 8, 3, pk, 0, None) == INVALID
    assert bands(po, 1, 0, 1, pk, 0, None) == INVALID
    assert bands(None, 1, 8, 2, pk, 0, None) == INVALID
    assert bands(po, 1, 8192, 2, pk, 0, None) == RANGE
    assert np.all(out == 0) and np.all(keys == 0)
    from custrings_amd import minhash

    with pytest.raises(ValueError):
        minhash.minhash(g, a=a)
    with pytest.raises(ValueError):
        minhash.minhash(g, width=300)
    with pytest.raises(ValueError):
        minhash.band_keys(np.zeros((2, 8), dtype=np.uint32), 3)
