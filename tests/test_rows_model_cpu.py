"""The Python model of find / contains / strip (tests/rows_model.py) against the oracle on every column and every parameter set
that tests/test_gpu_find_tile.py and tests/test_gpu_strip_tile.py run, results and counts, and every generator's plan: the tile
size and route its column was built for, restated from the offsets.  Proves the expected values with no GPU."""
import numpy as np
import pytest

import cpulibs
import rows_model as rm


@pytest.fixture(scope="module")
def orc():
    return cpulibs.Oracle()


def _first_row(col, a, b):
    bad = int(np.flatnonzero(np.asarray(a) != np.asarray(b))[0])
    return bad, col.rows[bad], a[bad], b[bad]


FIND_CASES = rm.find_cases()
STRIP_CASES = rm.strip_cases()


def check_find(orc, c, needle, windows):
    col = c.col()
    for st, en in windows:
        got, n = orc.find(col, needle, st, en)
        want, wn = rm.find_column(c.rows, needle, st, en)
        if not np.array_equal(got, want):
            raise AssertionError((needle, st, en) + _first_row(c, got, want))
        assert n == wn == int(np.count_nonzero(got != -1))
    got, n = orc.contains(col, needle)
    want, wn = rm.contains_column(c.rows, needle)
    assert np.array_equal(got, want) and n == wn, needle


@pytest.mark.parametrize("case", FIND_CASES, ids=[c.name for c in FIND_CASES])
def test_find_model_equals_oracle(orc, case):
    c = case.build()  # (asserts the column's plan)
    assert 0 < len(c.rows) <= 20_000
    assert rm.find_route(c, case.needle) == case.route
    check_find(orc, c, case.needle, case.windows)


def test_dense_then_sparse(orc):
    c = rm.col_dense_then_sparse(rm.MI355X_WORKGROUPS)
    assert len(c.rows) == 33_056
    for needle in (b"a", b"ab"):
        check_find(orc, c, needle, [(0, -1), (1, 96), (95, 200)])


def test_null_rows_and_empty_needle(orc):
    c = rm.Column([b"ab", None, b"", "é".encode()], held={1: b"ab"})
    for needle, want in ((b"", [-1, -2, -1, -1]), (b"ab", [0, -2, -1, -1])):
        assert rm.find_column(c.rows, needle)[0].tolist() == want == orc.find(c.col(), needle)[0].tolist()
    assert rm.find_column(c.rows, b"")[1] == 1  # the null row is counted
    assert rm.contains_column(c.rows, b"")[0].tolist() == [0, 0, 0, 0] == orc.contains(c.col(), b"")[0].tolist()


def test_the_model_refuses_a_window_that_ends_behind_the_row():
    assert rm.char_offset(b"\xc3\xc3\xa9ab", 2) == 4 and rm.char_offset(b"\xc3\xc3ab", 2) == 2 and rm.char_offset(b"\xf0\x80ab", 2) == 5
    with pytest.raises(rm.Undefined):
        rm.find(b"\xf0\x80ab", b"b", 0, 2)
    assert rm.find(b"\xf0\x80ab", b"b", 2, 200) == -1  # the start alone behind the row: no room for a hit
    assert rm.find(b"\xf0\x80ab", b"b", 1, 200) == -1 and rm.find(b"\xf0\x80ab", b"b", 0, 200) == 2


@pytest.mark.parametrize("case", STRIP_CASES, ids=[c.name for c in STRIP_CASES])
def test_strip_model_equals_oracle(orc, case):
    c = case.build()
    assert 0 < len(c.rows) <= 20_000
    col = c.col()
    for side in case.sides:
        got = orc.strip(col, rm.SETS[case.set_name], side)
        want = cpulibs.Col.from_list(rm.strip_column(c.rows, rm.SETS[case.set_name], side))
        if not got.same_as(want):
            a, b = got.to_bytes_list(), want.to_bytes_list()
            bad = next(i for i in range(len(a)) if a[i] != b[i])
            raise AssertionError((case.set_name, side, bad, c.rows[bad], a[bad], b[bad]))


def test_sets_are_what_their_names_say():
    sizes = {k: len(rm.DEFAULT_SET if v is None else v) for k, v in rm.SETS.items()}
    assert sizes["four"] == 4 and sizes["five"] == 5 and sizes["n64"] == 64 and sizes["n65"] == 65 and sizes["n200"] == 200
    assert all(len(set(v)) == len(v) for v in rm.SETS.values() if v)
    assert all(ord(ch) >= 0x80 for name in ("n64", "n65") for ch in rm.SETS[name])
    assert sum(ord(ch) >= 0x80 for ch in rm.SETS["n200"]) == 196  # 64 in the struct, 132 in `more`
    for name in rm.SETS:  # 'ü' and the other outsiders are in no set
        assert not set("".join(rm.OUTSIDE)) & set(rm.DEFAULT_SET if rm.SETS[name] is None else rm.SETS[name])


def test_plan_restates_the_thresholds():
    offs = lambda sizes: np.concatenate([[0], np.cumsum(sizes)])  # noqa: E731
    assert rm.plan(offs([96] * 63), "find").R == 64 and rm.plan(offs([96] * 64), "find").R == 32
    assert rm.plan(offs([191] * 64), "find").R == 32 and rm.plan(offs([192] * 64), "find").R == 16
    assert rm.plan(offs([382] * 64), "find").R == 16 and rm.plan(offs([383] * 64), "find").route == "rows"
    p = rm.plan(offs([383] * 64), "strip")
    assert (p.R, p.route, p.cap, p.oversize) == (64, "tile", 6128, [0])
    assert rm.plan(offs([95] * 64), "strip").oversize == [] and rm.plan(offs([]), "strip").route == "rows"
    assert rm.wave_ranges(9, 256) == [(t, t + 1) for t in range(9)] and rm.wave_ranges(1033, 256)[-1] == (1032, 1033)
    assert rm.find_route(rm.Column([b"ab"]), rm.NEEDLE65) == "rows" and rm.find_route(rm.Column([b"ab"]), rm.ascii_needle(64)) == "tile"


def test_windows_sit_on_the_word_boundaries():
    w = rm.windows_for(b"ab")
    assert {s for s, _ in w} == set(rm.STARTS)
    assert any(e < s for s, e in w) and any(e == s for s, e in w)
    for p in (0, 65, 94):  # one byte short of the hit's end, at it, one past it
        assert {(0, p + 1), (0, p + 2), (0, p + 3)} <= set(w)
    rows = rm.edge_rows(b"ab")
    assert {len(r) for r in rows} >= {0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96}
    assert {r.find(b"ab") for r in rows if len(r) == 96} >= {0, 1, 30, 31, 32, 33, 62, 63, 64, 65, 94}
