"""The case tables of test_gpu_arrays.py without a GPU: the model (arrays_model.py) and the oracle's restatement of the
reference agree exactly on every case, so the expectation the GPU file holds the library to is said twice, independently.
split_record / rsplit_record have one statement only, the oracle's: here it has to run every case of theirs."""
import pytest

import arrays_cases as AC
import arrays_model as M

TABLES = AC.all_tables()


def _check(case, orc):
    want = AC.run_model(case, orc)
    assert want is not None, case[0]
    assert AC.run_reference(case, orc) == want, case[0]
    return want


@pytest.mark.parametrize("table", sorted(TABLES))
def test_model_and_oracle_agree_on_table(oracle_engine, table):
    cases = TABLES[table]
    assert len({c[0] for c in cases}) == len(cases), "case ids repeat"
    for case in cases:
        _check(case, oracle_engine)


@pytest.mark.parametrize("name", AC.VARIANTS)
@pytest.mark.parametrize("n", AC.ROW_COUNTS)
def test_model_and_oracle_agree_on_shapes(oracle_engine, n, name):
    for case in AC.shape_cases(AC.variant(AC.rows_of(n), name)):
        _check(case, oracle_engine)


@pytest.mark.parametrize("name", sorted(AC.chains()))
def test_model_and_oracle_agree_along_chains(oracle_engine, name):
    first, steps = AC.chains()[name]
    cur = first
    for k, step in enumerate(steps):
        op, extra, args = step(cur)
        cols = [cur] + extra
        want = _check(("%s step %d %s" % (name, k, op), op, cols, args), oracle_engine)
        assert want != "raises"
        cur = AC.next_column(want)
    assert len(cur) > 0, "the chain ran empty"


def test_split_record_cases_all_have_an_expectation(oracle_engine):
    cases = AC.split_record_cases()
    assert len(cases) == 2 * len(AC.DELIMS) * len(AC.LIMITS)
    rows = len(AC.token_rows())
    for case in cases:
        flat, lst = AC.run_model(case, oracle_engine)
        assert len(lst) == rows + 1 and lst[0] == 0 and lst[-1] == len(flat), case[0]
        assert all(e is not None for e in flat), case[0]
        # a null row has no entries, every other row at least one (an empty string where it has no token)
        assert all((lst[r + 1] - lst[r] == 0) == (case[2][0][r] is None) for r in range(rows)), case[0]


def test_tables_hold_what_they_are_for():
    """the shapes the tables exist for are in them: a cheap guard against an edit that loses one"""
    assert AC.KBLOCK % 64 == 0 and AC.KBLOCK >= 128
    rows = AC.rows_of(AC.KBLOCK + 1)
    assert [i for i, r in enumerate(rows) if r is None] == [0, 63, 64, AC.KBLOCK]
    assert b"" in rows and any(r and len(r) == 1 for r in rows) and max(len(r) for r in rows if r) >= 5000
    assert any(r and b"\x00" in r for r in rows) and any(r and "😀".encode() in r for r in rows)
    wide = AC.wide_columns()
    assert len(wide) == 130 and all(len(c) == 70 for c in wide)
    assert wide[63][2] is None and wide[64][2] is not None and wide[127][5] is None and wide[128][5] is not None
    assert all(c[8] is not None for c in wide) and all(c[10] is None for c in wide)
    flat, lst = M.records(wide, True)
    assert [lst[r + 1] - lst[r] for r in range(11)] == [130, 0, 63, 64, 65, 127, 128, 129, 130, 63, 0]
    assert max(len(c) for _, _, cols, _ in AC.cat_cases() for c in [cols]) == M.CAT_MAX_COLUMNS
    assert [r.count(b"a") for r in AC.findall_rows(0) if r] == [k for k in AC.FINDALL_KS if k]
    assert AC.findall_rows(0) != AC.findall_rows(1) and sorted(map(repr, AC.findall_rows(0))) == sorted(map(repr, AC.findall_rows(1)))
