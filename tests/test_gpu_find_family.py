"""-m gpu: the find family through the C ABI -- find, contains, rfind, find_from, compare, startswith, endswith,
match_strings (the counted-rows route of cs_ops.hip) and find_multiple -- and the ngrams / join pair, exactly against the
oracle: every result AND the count each entry returns.  The count rule of every op is stated here once (COUNTED) and
applied to the expected array; the Python wrappers drop the count, so the entries are called directly."""
import ctypes as C

import numpy as np
import pytest

import cpulibs
import gpuutil

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257]  # a wave, a wave and a row, more than one workgroup
NEEDLE65 = "ab" * 32 + "c"  # 65 bytes: one more than the tile kernel of find / contains takes
# null and empty rows, characters of 2 and 4 bytes in front of a hit (positions count characters), a needle at both ends
# of a row, overlapping occurrences, rows shorter than the needle, and the 65-byte needle at the start, the end and inside
BLOCK = ["abxab", None, "", "aaaa", "éab", "😀ab😀", "a", "ab", "éé", "x😀é ab", "aa", "abab", "b", NEEDLE65, "x" + NEEDLE65,
         NEEDLE65 + "é", "ab" * 32, "é" + NEEDLE65 + "ab", None, "xyz", "aéa", "  ab"]
NEEDLES = ["ab", "aa", "é", "😀", "", "a", "abxabab", NEEDLE65]
BOUNDS = [(0, -1), (2, 5), (3, 2), (90, -1), (1, 200)]  # whole row, a window, an inverted window, a start beyond every row
FILL = 0x5A  # what a results buffer holds before the call

# which results an entry counts (null rows of the position ops hold -2 and are counted)
COUNTED = {
    "find": lambda v: v != -1,
    "rfind": lambda v: v != -1,
    "find_from": lambda v: v != -1,
    "compare": lambda v: v == 0,
    "startswith": lambda v: v != 0,
    "endswith": lambda v: v != 0,
    "contains": lambda v: v != 0,
    "match_strings": lambda v: v != 0,
}
DTYPE = {"find": np.int32, "rfind": np.int32, "find_from": np.int32, "compare": np.int32, "find_multiple": np.int32,
         "startswith": np.uint8, "endswith": np.uint8, "contains": np.uint8, "match_strings": np.uint8}


def rows_of(n):
    return [BLOCK[(i + i // len(BLOCK)) % len(BLOCK)] for i in range(n)]


def device(strs):
    from custrings_amd import nvstrings

    return nvstrings.to_device(strs)


def device_tiled(block, reps):
    """the column of `block`'s rows, `reps` times over"""
    one = cpulibs.Col.from_list(block)
    offsets = np.zeros(one.rows * reps + 1, dtype=np.int64)
    np.cumsum(np.tile(np.diff(one.offsets), reps), out=offsets[1:])
    bits = np.tile(np.array([x is not None for x in block], dtype=np.uint8), reps)
    return gpuutil.from_col(cpulibs.Col(np.tile(one.chars, reps), offsets, np.packbits(bits, bitorder="little")))


def call(op, n, *args, on_device=False):
    """cs_<op>(*args, results, on_device, stream, &count) with a results buffer of `n` items on the host or the device:
    (status, results as a host array, count); the buffer and the count start out with values no entry writes."""
    import torch

    L = gpuutil.lib().lib
    fn = getattr(L, "cs_" + op)
    count = C.c_int64(-77)
    fill = FILL if DTYPE[op] == np.uint8 else FILL * 0x01010101
    if on_device:
        t = torch.full((max(n, 1),), fill, dtype=torch.uint8 if DTYPE[op] == np.uint8 else torch.int32, device="cuda")
        st = fn(*args, t.data_ptr(), 1, None, C.byref(count))
        torch.cuda.synchronize()
        res = t.cpu().numpy()
    else:
        res = np.full(max(n, 1), fill, dtype=DTYPE[op])
        st = fn(*args, res.ctypes.data, 0, None, C.byref(count))
    return st, res, count.value


def untouched(res):
    return bool(np.all(res.view(np.uint8) == FILL))


def check(op, expect, n, *args, on_device=False, what=None, route=None):
    expect = np.asarray(expect, dtype=DTYPE[op])
    st, res, count = call(op, n, *args, on_device=on_device)
    assert st == 0, (op, what)
    if route is not None:
        assert gpuutil.lib().lib.cs_debug_last_route().decode() == route, (op, what)
    assert np.array_equal(res[:n], expect), (op, what)
    assert count == int(np.count_nonzero(COUNTED[op](expect))), (op, what, "count")
    if n == 0:
        assert untouched(res), (op, what)


def compare_expected(o, s, sub):
    """(the reference returns from compare("") without writing, and the oracle follows it; the C ABI compares with the empty
    string like with any other: 1 for a non-empty row, 0 for an empty one, -1 for a null one)"""
    if sub == "":
        return [-1 if x is None else (1 if x else 0) for x in s]
    return o.compare(s, sub)[0]


def check_needle_ops(o, g, s, sub, on_device=False):
    """the one-needle entries that have one route"""
    n, b = len(s), sub.encode("utf8")
    for st, en in BOUNDS + [(-3, -1), (-2, 4)]:  # (rfind takes a negative start as 0)
        check("rfind", o.rfind(s, sub, st, en)[0], n, g.m_cptr, b, st, en, on_device=on_device, what=(sub, st, en))
    check("compare", compare_expected(o, s, sub), n, g.m_cptr, b, on_device=on_device, what=sub)
    check("startswith", o.startswith(s, sub)[0], n, g.m_cptr, b, on_device=on_device, what=sub)
    check("endswith", o.endswith(s, sub)[0], n, g.m_cptr, b, on_device=on_device, what=sub)


def bounds_for(n):
    starts = np.array([(-2, 0, 1, 2, 3, 5, 40, 100)[i % 8] for i in range(n)], dtype=np.int32)
    ends = np.array([(-1, 0, 2, 4, 5, 7, 66, 200, -2)[i % 9] for i in range(n)], dtype=np.int32)
    return starts, ends


def check_find_from(o, g, s, sub, bounds_on_device):
    import torch

    n, b = len(s), sub.encode("utf8")
    starts, ends = bounds_for(n)
    for a, e in ((None, None), (starts, None), (None, ends), (starts, ends)):
        keep = [None if x is None else torch.from_numpy(x).cuda() for x in (a, e)] if bounds_on_device else [a, e]
        pa, pe = [None if x is None else (x.data_ptr() if bounds_on_device else x.ctypes.data) for x in keep]
        check("find_from", o.find_from(s, sub, a, e)[0], n, g.m_cptr, b, pa, pe, 1 if bounds_on_device else 0,
              what=(sub, a is None, e is None, bounds_on_device))


def route_of(n, needle, rowwise):
    """the route find / contains must report on the rows of BLOCK (every tile of them fits the staging buffer): the tile
    kernel takes needles of up to 64 bytes, the empty one too; no rows: the entry returns before it takes one"""
    if n == 0:
        return None
    return "rows" if rowwise or len(needle) > 64 else "tile"


@pytest.mark.parametrize("rowwise", [False, True], ids=["default", "rowwise"])
@pytest.mark.parametrize("n", SIZES)
def test_find_and_contains_on_both_routes(oracle_engine, monkeypatch, n, rowwise):
    if rowwise:
        monkeypatch.setenv("CS_FIND_ROWWISE", "1")
    s = rows_of(n)
    g = device(s)
    for sub in NEEDLES:
        b = sub.encode("utf8")
        route = route_of(n, b, rowwise)
        for st, en in BOUNDS:
            check("find", oracle_engine.find(s, sub, st, en)[0], n, g.m_cptr, b, st, en, what=(sub, st, en), route=route)
        check("contains", oracle_engine.contains(s, sub)[0], n, g.m_cptr, b, what=sub, route=route)


@pytest.mark.parametrize("n", SIZES)
def test_one_route_entries(oracle_engine, n):
    o = oracle_engine
    s = rows_of(n)
    g = device(s)
    for sub in NEEDLES:
        check_needle_ops(o, g, s, sub)
        check_find_from(o, g, s, sub, False)
    other = [x if i % 3 else (None if i % 2 else (x or "") + "x") for i, x in enumerate(s)]  # every third row differs: a null or a longer row
    for t in (s, other):
        other_col = device(t)  # (held: the entry gets its address)
        check("match_strings", o.match_strings(s, t)[0], n, g.m_cptr, other_col.m_cptr, what="match_strings")
    targets = ["ab", "é", None, "", NEEDLE65]
    gt = device(targets)
    want, want_n = o.find_multiple(s, targets)
    st, res, count = call("find_multiple", n * len(targets), g.m_cptr, gt.m_cptr)
    assert st == 0 and res[:n * len(targets)].tolist() == want and count == want_n
    assert count == sum(1 for v in want[:n] if v != -1)  # (the reference's count looks at the first rows() entries)


def test_results_and_bounds_in_device_memory(oracle_engine, monkeypatch):
    o = oracle_engine
    s = rows_of(257)
    n = len(s)
    g = device(s)
    for rowwise in (False, True):
        if rowwise:
            monkeypatch.setenv("CS_FIND_ROWWISE", "1")
        for sub in ("ab", "é", NEEDLE65):
            b = sub.encode("utf8")
            route = route_of(n, b, rowwise)
            check("find", o.find(s, sub, 1, 40)[0], n, g.m_cptr, b, 1, 40, on_device=True, what=(sub, rowwise), route=route)
            check("contains", o.contains(s, sub)[0], n, g.m_cptr, b, on_device=True, what=(sub, rowwise), route=route)
    for sub in ("ab", "", "😀"):
        check_needle_ops(o, g, s, sub, on_device=True)
        check_find_from(o, g, s, sub, True)
    starts, ends = bounds_for(n)
    check("find_from", o.find_from(s, "ab", starts, ends)[0], n, g.m_cptr, b"ab", starts.ctypes.data, ends.ctypes.data, 0, on_device=True)
    other_col = device(s[1:] + s[:1])  # (held: the entry gets its address)
    check("match_strings", o.match_strings(s, s[1:] + s[:1])[0], n, g.m_cptr, other_col.m_cptr, on_device=True)
    targets = ["ab", None, "a"]
    want, want_n = o.find_multiple(s, targets)
    other_col = device(targets)  # (held: the entry gets its address)
    st, res, count = call("find_multiple", n * 3, g.m_cptr, other_col.m_cptr, on_device=True)
    assert st == 0 and res.tolist() == want and count == want_n


def test_more_rows_than_one_grid_of_threads(oracle_engine, monkeypatch):
    """Above 8192 workgroups of 256 rows the threads go round their loop again: a 4099-row block 512 times (2 098 688 rows);
    what the oracle says of the block, 512 times, is what the column must give."""
    o = oracle_engine
    reps = 512
    block = rows_of(4099)
    for i in range(0, 4099, 5):  # rows of a few bytes
        block[i] = ("ab", None, "é", "xaab")[i // 5 % 4]
    block = [x if x is None or len(x) < 12 else x[:3] for x in block]
    n = len(block) * reps
    assert n > 8192 * 256
    g = device_tiled(block, reps)
    assert g.size() == n

    def tiled(expect):
        return np.tile(np.asarray(expect), reps)

    monkeypatch.setenv("CS_FIND_ROWWISE", "1")
    check("find", tiled(o.find(block, "ab", 1, -1)[0]), n, g.m_cptr, b"ab", 1, -1)
    check("contains", tiled(o.contains(block, "ab")[0]), n, g.m_cptr, b"ab")
    check("rfind", tiled(o.rfind(block, "a", 0, -1)[0]), n, g.m_cptr, b"a", 0, -1)
    starts = np.array([i % 3 for i in range(4099)], dtype=np.int32)
    big_starts = np.tile(starts, reps)
    check("find_from", tiled(o.find_from(block, "ab", starts, None)[0]), n, g.m_cptr, b"ab", big_starts.ctypes.data, None, 0)
    check("compare", tiled(o.compare(block, "ab")[0]), n, g.m_cptr, b"ab")
    check("startswith", tiled(o.startswith(block, "ab")[0]), n, g.m_cptr, b"ab")
    check("endswith", tiled(o.endswith(block, "ab")[0]), n, g.m_cptr, b"ab")
    other = list(block)
    other[7], other[4098] = "zz", None
    other_col = device_tiled(other, reps)  # (held: the entry gets its address)
    check("match_strings", tiled(o.match_strings(block, other)[0]), n, g.m_cptr, other_col.m_cptr)


def test_a_column_without_a_hit_returns_zero(oracle_engine, monkeypatch):
    s = ["ab", "", "é", "xyz"] * 70  # (no null row: the position entries count those)
    n = len(s)
    g = device(s)
    for rowwise in (False, True):
        if rowwise:
            monkeypatch.setenv("CS_FIND_ROWWISE", "1")
        check("find", [-1] * n, n, g.m_cptr, b"q", 0, -1)
        check("contains", [0] * n, n, g.m_cptr, b"q")
    check("rfind", [-1] * n, n, g.m_cptr, b"q", 0, -1)
    check("find_from", [-1] * n, n, g.m_cptr, b"q", None, None, 0)
    check("startswith", [0] * n, n, g.m_cptr, b"q")
    check("endswith", [0] * n, n, g.m_cptr, b"q")
    st, res, count = call("compare", n, g.m_cptr, b"q")
    assert st == 0 and count == 0 and not np.any(res == 0)
    other_col = device(["q"] * n)  # (held: the entry gets its address)
    check("match_strings", [0] * n, n, g.m_cptr, other_col.m_cptr)
    # and null rows alone are what the position entries count then
    h = device(["ab", None, "", None])
    check("find", [-1, -2, -1, -2], 4, h.m_cptr, b"q", 0, -1)
    check("rfind", [-1, -2, -1, -2], 4, h.m_cptr, b"q", 0, -1)
    check("find_from", [-1, -2, -1, -2], 4, h.m_cptr, b"q", None, None, 0)
    check("compare", oracle_engine.compare(["ab", None, "", None], "q")[0], 4, h.m_cptr, b"q")


def test_argument_rules():
    from custrings_amd import _lib

    g = device(["ab", None, "b"])
    e = device([])
    st, res, count = call("contains", 3, g.m_cptr, None)
    assert st == _lib.CS_ERR_INVALID_ARG and count == -1 and untouched(res)
    for args in ((None, g.m_cptr), (g.m_cptr, None)):
        st, res, count = call("match_strings", 3, *args)
        assert st == _lib.CS_ERR_INVALID_ARG and count == -1 and untouched(res)
    other_col = device(["ab", None])  # (held: the entry gets its address)
    st, res, count = call("match_strings", 3, g.m_cptr, other_col.m_cptr)
    assert st == _lib.CS_ERR_INVALID_ARG and untouched(res)
    L = _lib.lib
    count = C.c_int64(-77)
    assert L.cs_contains(g.m_cptr, b"a", None, 0, None, C.byref(count)) == _lib.CS_ERR_INVALID_ARG and count.value == -1
    assert L.cs_match_strings(g.m_cptr, g.m_cptr, None, 0, None, C.byref(count)) == _lib.CS_ERR_INVALID_ARG and count.value == -1
    # the others say nothing: status 0, count 0, nothing written -- for no column, no needle and no rows
    silent = {
        "find": lambda c, s: (c, s, 0, -1),
        "rfind": lambda c, s: (c, s, 0, -1),
        "find_from": lambda c, s: (c, s, None, None, 0),
        "compare": lambda c, s: (c, s),
        "startswith": lambda c, s: (c, s),
        "endswith": lambda c, s: (c, s),
    }
    for op, args in silent.items():
        for c, s in ((None, b"a"), (g.m_cptr, None), (e.m_cptr, b"a")):
            for on_device in (False, True):
                st, res, count = call(op, 3, *args(c, s), on_device=on_device)
                assert st == 0 and count == 0 and untouched(res), (op, c is None, s is None, on_device)
        count = C.c_int64(-77)
        assert getattr(L, "cs_" + op)(*args(g.m_cptr, b"a"), None, 0, None, C.byref(count)) == 0 and count.value == 0, op
    t = device(["a"])
    for c, o in ((None, t.m_cptr), (g.m_cptr, None), (e.m_cptr, t.m_cptr), (g.m_cptr, e.m_cptr)):
        st, res, count = call("find_multiple", 3, c, o)
        assert st == 0 and count == 0 and untouched(res)
    for op, args in (("contains", (e.m_cptr, b"a")), ("match_strings", (e.m_cptr, e.m_cptr))):  # (no rows: no error either)
        st, res, count = call(op, 0, *args)
        assert st == 0 and count == 0 and untouched(res)


@pytest.mark.parametrize("sep", ["", "_", "é"])
@pytest.mark.parametrize("n", [2, 3])
def test_ngrams_of_few_tokens_are_their_join(gpu_engine, oracle_engine, n, sep):
    """create_ngrams drops null and empty rows; with no more than n left it answers join(separator, "") of ALL rows"""
    g, o = gpu_engine, oracle_engine
    words = ["tok", "é", "b😀", "zz", "q"]
    for kept in (n - 1, n, n + 1):
        for toks in (words[:kept],  # nothing dropped
                     [None, ""] + [x for w in words[:kept] for x in (w, None, "")],
                     [x for w in words[:kept] for x in ("", w)] + [None]):
            got = g.ngrams(toks, n, sep)
            assert got == o.ngrams(toks, n, sep), (kept, toks)
            if kept <= n:
                joined = o.join(toks, sep, "")
                assert got == joined and g.join(toks, sep, "") == joined, (kept, toks)
            else:
                assert len(got) == 2 and got[0] == sep.join(words[:n])
    # join by itself: null rows without a replacement leave no delimiter either
    toks = [None, "a", "", None, "é", None]
    for narep in (None, "", "<n>"):
        assert g.join(toks, sep, narep) == o.join(toks, sep, narep), narep
