"""find / contains on the MI355X against the oracle and the Python model of tests/rows_model.py, with the route proven
(cs_debug_last_route): k_find_tile (cs_rows.hip) on ASCII rows whose sizes, hits and windows sit on the 32-bit words of its
candidate bitmap, tiles of the bit path next to tiles that walk their rows, multi-byte characters in front of a hit, a sparse
tile behind a dense one on the same wave, the three tile sizes at partial tiles and partial workgroups, arbitrary bytes, and
borrowed columns whose chars start inside a 16-byte piece.  tests/test_rows_model_cpu.py proves the expected values.

Every comparison is exact: the result array (the buffer prefilled with a pattern) and the returned count, against both; the
route is the one the case's table fixes; the input's digest and the fallback count do not move; every "tile" case runs once
more with CS_FIND_ROWWISE, where the route is "rows" and the output the same."""
import ctypes as C

import numpy as np
import pytest

import borrowedutil as bu
import cpulibs
import gpuutil
import rows_model as rm

pytestmark = pytest.mark.gpu

FILL = 0x5A
FIND_CASES = rm.find_cases()


@pytest.fixture(scope="module")
def orc():
    return cpulibs.Oracle()


def run(op, g, needle, start=0, end=-1):
    """-> (results, count, route) of cs_find / cs_contains into a prefilled host buffer"""
    L = gpuutil.lib().lib
    count = C.c_int64(-77)
    if op == "find":
        res = np.full(g.size(), FILL * 0x01010101, dtype=np.int32)
        st = L.cs_find(g.m_cptr, needle, start, end, res.ctypes.data, 0, None, C.byref(count))
    else:
        res = np.full(g.size(), FILL, dtype=np.uint8)
        st = L.cs_contains(g.m_cptr, needle, res.ctypes.data, 0, None, C.byref(count))
    assert st == 0
    return res, count.value, L.cs_debug_last_route().decode()


def same(got, refs, column, what):
    res, count, took = got
    for name, (want, n) in refs.items():
        if not np.array_equal(res, want):
            bad = int(np.flatnonzero(res != want)[0])
            raise AssertionError(what + (took, name, "row", bad, column.rows[bad], "got", int(res[bad]), "want", int(want[bad])))
        assert count == n, what + (took, name, "count", count, n)


def check(orc, monkeypatch, column, needle, windows, route, g=None):
    L = gpuutil.lib()
    col = column.col()
    g = g if g is not None else gpuutil.from_col(col)
    before, f0 = g.digest(), L.lib.cs_fallback_count()
    expect = {}
    for st, en in windows:
        expect["find", st, en] = {"oracle": orc.find(col, needle, st, en), "model": rm.find_column(column.rows, needle, st, en)}
    expect["contains", 0, -1] = {"oracle": orc.contains(col, needle), "model": rm.contains_column(column.rows, needle)}
    for rowwise in (False, True):
        if rowwise:
            if route != "tile":
                break
            monkeypatch.setenv("CS_FIND_ROWWISE", "1")
        for (op, st, en), refs in expect.items():
            got = run(op, g, needle, st, en)
            assert got[2] == ("rows" if rowwise else route), (op, needle, st, en, got[2])
            same(got, refs, column, (op, needle, st, en))
    monkeypatch.delenv("CS_FIND_ROWWISE", raising=False)
    assert g.digest() == before and L.lib.cs_fallback_count() == f0


@pytest.mark.parametrize("case", FIND_CASES, ids=[c.name for c in FIND_CASES])
def test_find_and_contains(orc, monkeypatch, case):
    """the table of tests/rows_model.py::find_cases: edge rows and windows on the bitmap's words for needles of 1 to 64
    bytes (65: the row kernels), ASCII tiles next to tiles with an 'é', a 97-byte row, multi-byte characters in front of the
    hit, 64-, 32- and 16-row tiles at row counts around a tile and a workgroup, and arbitrary bytes"""
    check(orc, monkeypatch, case.build(), case.needle, case.windows, case.route)


def test_sparse_tile_behind_a_dense_one(orc, monkeypatch):
    """tiles of 96-byte rows of 'a' in front of tiles of short rows and of null and empty rows, walked by the same wave: the
    launch is held to one workgroup a compute unit, and the column has more tiles than that launch has waves"""
    import torch

    workgroups = torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.setenv("CS_STREAM_BLOCKS_PER_CU", "1")
    column = rm.col_dense_then_sparse(workgroups)  # (asserts from the plan that a wave walks D-S and D-N)
    for needle in (b"a", b"ab"):
        check(orc, monkeypatch, column, needle, [(0, -1), (1, 96), (95, 200)], "tile")


@pytest.mark.parametrize("shift", [1, 7, 13])
@pytest.mark.parametrize("shape,n", [("R64", 300), ("R32", 300), ("R16", 1000)])
def test_shifted_chars_buffer(orc, monkeypatch, shape, n, shift):
    """a borrowed column whose chars start `shift` bytes past a 16-byte boundary, 0xFF bytes around: every tile's `lead`
    moves, and the bits of the bytes in front of the column are no row's"""
    column = rm.col_find_shape(shape, n).check_plan(base=shift)
    b = bu.Borrowed(column.rows, shift, 8, bu.poison_for("ff", "text"))
    check(orc, monkeypatch, column, b"ab", [(0, -1), (3, 50)], "tile", g=b.col)
    assert b.caller_memory_intact()
