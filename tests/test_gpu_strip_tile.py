"""strip / lstrip / rstrip on the MI355X against the oracle and the Python model of tests/rows_model.py, with the route proven
(cs_debug_last_route): the write pass k_strip_tile (cs_rows.hip) with sets of one to 200 characters, rows stripped on either
end, to nothing and not at all, the three tile sizes at a partial last tile, output tiles at every destination alignment and
tiles without output, tiles beyond the staging buffer with rows on both sides of the lane-copy / wave-copy switch, arbitrary
bytes, and borrowed columns whose chars start inside a 16-byte piece.  tests/test_rows_model_cpu.py proves the expected values.

Every comparison is byte-exact on chars, int64 offsets and validity, against both; the route is the one the case's table
fixes; the input's digest and the fallback count do not move; every case runs once more with CS_STRIP_ROWWISE, where the
route is "rows" and the output the same."""
import numpy as np
import pytest

import borrowedutil as bu
import cpulibs
import gpuutil
import rows_model as rm

pytestmark = pytest.mark.gpu

STRIP_CASES = rm.strip_cases()


@pytest.fixture(scope="module")
def orc():
    return cpulibs.Oracle()


def same(got, want, column, what):
    assert got.rows == want.rows, what
    assert np.array_equal(got.bitmask(), want.bitmask()), what + ("validity",)
    if not (np.array_equal(got.offsets, want.offsets) and np.array_equal(got.chars, want.chars)):
        a, b = got.to_bytes_list(), want.to_bytes_list()
        bad = next((i for i in range(len(a)) if a[i] != b[i]), None)
        if bad is None:
            raise AssertionError(what + ("offsets",))
        raise AssertionError(what + ("row", bad, (column.rows[bad] or b"")[:96], "got", (a[bad] or b"")[:96], "want", (b[bad] or b"")[:96]))


def check(orc, monkeypatch, column, set_name, sides, route, g=None):
    L = gpuutil.lib()
    col = column.col()
    g = g if g is not None else gpuutil.from_col(col)
    chars = rm.SETS[set_name]
    before, f0 = g.digest(), L.lib.cs_fallback_count()
    expect = {side: {"oracle": orc.strip(col, chars, side), "model": cpulibs.Col.from_list(rm.strip_column(column.rows, chars, side))}
              for side in sides}
    for rowwise in (False, True):
        if rowwise:
            monkeypatch.setenv("CS_STRIP_ROWWISE", "1")
        for side, refs in expect.items():
            out = g._strip(chars, side)
            took = L.lib.cs_debug_last_route().decode()
            assert took == ("rows" if rowwise else route), (set_name, side, took)
            got = gpuutil.to_col(out)  # (_export64: int64 offsets)
            for name, want in refs.items():
                same(got, want, column, (set_name, side, took, name))
    monkeypatch.delenv("CS_STRIP_ROWWISE", raising=False)
    assert g.digest() == before and L.lib.cs_fallback_count() == f0


@pytest.mark.parametrize("case", STRIP_CASES, ids=[c.name for c in STRIP_CASES])
def test_strip(orc, monkeypatch, case):
    """the table of tests/rows_model.py::strip_cases: every set on its rows, the three tile sizes, the sixteen destination
    alignments with tiles that strip to nothing, the tiles beyond the staging buffer, and arbitrary bytes with five sets"""
    check(orc, monkeypatch, case.build(), case.set_name, case.sides, case.route)


@pytest.mark.parametrize("shift", [1, 7, 13])
@pytest.mark.parametrize("shape,n", [("R64", 64 * 3 + 7), ("R32", 32 * 5 + 9), ("R16", 16 * 7 + 3)])
def test_shifted_chars_buffer(orc, monkeypatch, shape, n, shift):
    """a borrowed column whose chars start `shift` bytes past a 16-byte boundary, 0xFF bytes around: every tile's `lead`
    moves, and with it which tiles fill their staging buffer to the last 48 bytes"""
    rows = rm.col_strip_shape(shape, n).rows  # (a null row of a borrowed column spans no bytes)
    column = rm.Column(rows, want_strip=(int(shape[1:]), "tile")).check_plan(base=shift)
    b = bu.Borrowed(column.rows, shift, 8, bu.poison_for("ff", "text"))
    check(orc, monkeypatch, column, "e_acute_", (0, 1, 2), "tile", g=b.col)
    assert b.caller_memory_intact()
