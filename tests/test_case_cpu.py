"""The Python model of lower / upper (tests/case_model.py) against the oracle on every column the GPU tests of
tests/test_gpu_case.py build from it, and the conditions those columns have to meet.  No GPU."""
import numpy as np
import pytest

import case_model as cm
import chartype_model as m
import cpulibs


@pytest.fixture(scope="module")
def orc():
    return cpulibs.Oracle()


def _same(orc, op, rows):
    col = cpulibs.Col.from_list(rows)
    got = getattr(orc, op)(col)
    want = cpulibs.Col.from_list(cm.case_column(op, rows))
    if not got.same_as(want):
        a, b = got.to_bytes_list(), want.to_bytes_list()
        bad = next(i for i in range(len(rows)) if a[i] != b[i])
        raise AssertionError((op, bad, rows[bad], a[bad], b[bad]))


@pytest.mark.parametrize("op", cm.OPS)
@pytest.mark.parametrize("gen", ["singles", "embedded", "packed"])
def test_model_equals_oracle_on_keepers(orc, op, gen):
    rows = getattr(cm, gen)(op)
    assert 0 < len(rows) < 70_000
    _same(orc, op, rows)
    _same(orc, op, cm.with_nulls(rows))
    # a keeper column keeps every row's size: the condition of the tile route
    assert all(len(r.encode()) == len(cm.case_row(op, r).encode()) for r in rows)


@pytest.mark.parametrize("op", cm.OPS)
def test_model_equals_oracle_on_changers(orc, op):
    rows = cm.changer_column(op)
    _same(orc, op, rows)
    assert all(len(r.encode()) != len(cm.case_row(op, r).encode()) for r in rows)


def test_keepers_and_changers_partition_the_cased_set():
    flags, _ = m.tables()
    every = set(range(0x80, 0x10000)) - set(range(0xD800, 0xE000))
    cased = set(cm.cased())
    assert len(cased) == 2622 and sum(cp >= 0x800 for cp in cased) == 1617  # (the table's cased non-ASCII code points)
    assert not cased & set(range(0xD800, 0xE000))
    for op in cm.OPS:
        keep, change = set(cm.keepers(op)), set(cm.changers(op))
        assert not keep & change and keep | change == every
        assert change <= cased and all(flags[cp] & cm.BITS[op] for cp in change)
        assert cased == (cased & keep) | change
    both = set(cm.changers("lower")) | set(cm.changers("upper"))
    assert len(both) == 98  # DESIGN.md, section chartype
    assert both == set(m.width_changing()) - set(range(0x80))


def test_packed_rows_start_at_every_phase():
    for op in cm.OPS:
        rows = cm.packed(op)
        starts = np.cumsum([0] + [len(r.encode()) for r in rows])[:-1]
        assert set((starts % 16).tolist()) == set(range(16)) and set((starts % 32).tolist()) == set(range(32))
        assert not any(ord(ch) < 0x80 for r in rows for ch in r)
        assert sum(cm.FOUR_BYTE[0] in r and cm.FOUR_BYTE[1] in r for r in rows) >= 50


def test_size_keeping_bytes_conditions(orc):
    """the generator asserts its own conditions (1,000 malformed rows, 1,000 rows that an ASCII flip gets wrong); here: what
    it returns is what the oracle says, sizes kept, and the rows with a truncated last character are among the kept ones"""
    kept, low, up = cm.size_keeping_bytes(7, 40_000, orc)
    assert 10_000 < len(kept) < 70_000
    col = cpulibs.Col.from_list(kept)
    assert orc.lower(col).same_as(cpulibs.Col.from_list(low)) and orc.upper(col).same_as(cpulibs.Col.from_list(up))
    assert np.array_equal(orc.lower(col).offsets, col.offsets) and np.array_equal(orc.upper(col).offsets, col.offsets)
    bad = [i for i, r in enumerate(kept) if not cm.is_utf8(r)]
    assert len(bad) >= 1000
    assert sum(low[i] != kept[i].lower() for i in bad) >= 1000
    assert sum(up[i] != kept[i].upper() for i in bad) >= 1000
    crafted = set(cm.truncated_tails())
    tails = [i for i, r in enumerate(kept) if r in crafted and not r.isascii()]
    assert len(tails) >= 18 * 4, len(tails)
    assert all(kept[i + 1].isascii() for i in tails)  # (the row a character running past its row would damage)
    # the rows' malformed output is not the input with its ASCII letters flipped: a kernel that skipped them would show
    assert sum(low[i] != kept[i].lower() for i in tails) == len(tails)
