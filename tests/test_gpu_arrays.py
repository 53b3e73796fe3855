"""-m gpu: the array, combine, record and partition ops (cs_array.hip, cs_records.hip) at their batch and shape edges,
against the model (arrays_model.py; the oracle for split_record / rsplit_record): the cases of arrays_cases.py, which
test_arrays_cpu.py holds the model and the oracle to.  Compared byte for byte -- chars, offsets, which rows are null, the list
offsets -- through the flat forms.

What the shapes are for: records_from_columns beyond its first batch of 64 columns (k_record_counts' carry, the entries at
e0 + k0 + j), cat at its 16 columns, the four walks of record_tokens with limits and delimiters running out in either order
and delimiters that are multi-byte, overlap themselves or exceed the row, rfind for rpartition, row counts at the workgroup
(kBlock) and bitmask-word edges, input columns without a bitmask / all null / windows of longer columns / results of earlier
ops, k_scatter_select's several writers of one row, and k_gather_lengths' bad position in any lane."""
import numpy as np
import pytest

import arrays_cases as AC
import arrays_model as M

pytestmark = pytest.mark.gpu

KINDS = ["bitmask", "no_bitmask", "all_null", "offsets64", "window", "result_of_gather"]
VARIANT_OF = {"no_bitmask": "no_nulls", "all_null": "all_null"}


@pytest.fixture(scope="module")
def nvs(gpu_engine):
    return gpu_engine.nvs


def _offsets64(nvs, rows):
    """from_offsets64 of the rows: with a bitmask when a row is null, with none at all when none is (NUL bytes or not --
    to_device would give a row with a NUL byte an all-ones bitmask)"""
    lens = np.array([0 if r is None else len(r) for r in rows], dtype=np.int64)
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = np.frombuffer(b"".join(r for r in rows if r is not None) or b"\0", dtype=np.uint8)
    valid = None
    if any(r is None for r in rows):
        bits = np.packbits(np.array([r is not None for r in rows], dtype=np.uint8), bitorder="little")
        valid = np.concatenate([bits, np.zeros(8, dtype=np.uint8)])
    return nvs.from_offsets64(chars, offs, len(rows), valid)


def has_bitmask(col):
    """whether the device column carries a validity bitmask (a null pointer stands for "every row valid")"""
    import ctypes as C

    from custrings_amd import _lib

    v = _lib.ColumnView()
    _lib.check(_lib.lib.cs_column_get_view(col.m_cptr, C.byref(v)))
    return bool(v.validity)


def column(nvs, rows, kind="bitmask"):
    """the same logical rows as a device column of the given kind; rows without a null among them make a column without a
    bitmask whatever the kind (but a window or a gather of a column that has one)"""
    if kind == "no_bitmask" or (kind in ("bitmask", "offsets64") and rows and all(r is not None for r in rows)):
        assert all(r is not None for r in rows)
        col = _offsets64(nvs, rows)
        assert not rows or not has_bitmask(col)
        return col
    if kind in ("bitmask", "all_null"):
        return nvs.to_device(rows)
    if kind == "offsets64":
        return _offsets64(nvs, rows)
    if kind == "window":
        # rows 67 .. 67 + n of a longer column: cs_column_slice reads the longer column's offsets from a first one that is not
        # 0 and its bitmask from the middle of a word, and hands out a rebased copy (offsets from 0, bitmask from bit 0)
        longer = [b"before%d" % i if i % 5 else None for i in range(67)] + list(rows) + [None, b"after"]
        return nvs.to_device(longer).sublist(67, 67 + len(rows))
    assert kind == "result_of_gather"
    return nvs.to_device(rows[::-1]).gather(list(range(len(rows) - 1, -1, -1)))


def host(col):
    """device column -> list of bytes / None; the offsets start at 0 and a null row has no bytes"""
    chars, offs, valid = col._export64()
    rows = len(offs) - 1
    assert rows == col.size() and int(offs[0]) == 0 and int(offs[-1]) == len(chars)
    bits = np.unpackbits(valid, bitorder="little")[:rows]
    data, o = chars.tobytes(), offs.tolist()
    assert all(bits[i] or o[i] == o[i + 1] for i in range(rows)), "a null row holds bytes"
    return [data[o[i]:o[i + 1]] if bits[i] else None for i in range(rows)]


def run_gpu(nvs, op, g, args):
    """the library's side of a case on device columns `g`: (plain result as arrays_cases states them, the result column)"""
    c = g[0] if g else None
    rec = None
    if op == "gather":
        out = c.gather(list(args[0]))
    elif op == "gather_mask":
        out = c.gather([bool(m) for m in args[0]])
    elif op == "remove_strings":
        out = c.remove_strings(list(args[0]))
    elif op == "sublist":
        out = c.sublist(*args)
    elif op == "scatter":
        out = c.scatter(g[1], list(args[0]))
    elif op == "scalar_scatter":
        out = c.scalar_scatter(args[0], list(args[1]), len(args[1]))
    elif op == "cat":
        out = c.cat(g[1:], args[0], args[1])
    elif op == "join":
        out = c.cat(None, args[0], args[1])
    elif op == "order":
        return c.order(*args), None
    elif op == "sort":
        out = c.sort(*args)
    elif op == "records":
        out, rec = nvs.nvstrings._records(g, args[0])
    elif op == "split_then_records":
        out, rec = nvs.nvstrings._records(c.split(args[0]), args[1])
    elif op == "findall_record":
        out, rec = c.findall_record(args[0], flat=True)
    elif op in ("split_record", "rsplit_record"):
        out, rec = getattr(c, op)(args[0], args[1], flat=True)
    elif op in ("partition", "rpartition"):
        out = getattr(c, op)(args[0], flat=True)
        rec = np.arange(0, 3 * c.size() + 1, 3)
    else:
        raise KeyError(op)
    return (host(out) if rec is None else (host(out), [int(v) for v in rec])), out


def gpu_outcome(nvs, op, g, args):
    try:
        return run_gpu(nvs, op, g, args)
    except (ValueError, IndexError):
        return "raises", None


def check(nvs, case, orc, kind="bitmask"):
    name, op, cols, args = case
    want = AC.run_model(case, orc)
    g = [column(nvs, cols[0], kind)] + [column(nvs, c) for c in cols[1:]] if cols else []
    if "without_bitmask" in name:
        assert not has_bitmask(g[0]), name
    got, out = gpu_outcome(nvs, op, g, args)
    assert got == want, (name, kind)
    return out


# ---- every op on every kind of input column, at the workgroup and bitmask-word edges ------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", AC.ROW_COUNTS)
def test_gpu_ops_on_each_column_kind_at_block_edges(nvs, oracle_engine, n, kind):
    rows = AC.variant(AC.rows_of(n), VARIANT_OF.get(kind, "as_is"))
    probe = column(nvs, rows, kind)
    assert host(probe) == rows
    assert (probe.size(), probe.null_count(), probe.byte_count()) == M.metadata(rows)
    if kind in ("bitmask", "no_bitmask", "all_null", "offsets64"):
        assert has_bitmask(probe) == (kind != "no_bitmask"), "the column is not of the kind it is named for"
    if kind == "no_bitmask":  # an op that shares or drops the input's validity keeps the column without one
        part = probe.partition(b" ", flat=True)
        assert not has_bitmask(probe.gather([0])) and not has_bitmask(part) and part.null_count() == 0
    for case in AC.shape_cases(rows):
        check(nvs, case, oracle_engine, kind)


# ---- the tables ------------------------------------------------------------------------------------------------------------
TABLES = AC.all_tables()


@pytest.mark.parametrize("table", sorted(TABLES))
def test_gpu_table(nvs, oracle_engine, table):
    for case in TABLES[table]:
        check(nvs, case, oracle_engine)


def test_gpu_wide_records_on_each_column_kind(nvs, oracle_engine):
    """the 130 columns again, each column of another kind than its neighbour"""
    wide = AC.wide_columns()
    g = [column(nvs, c, KINDS[k % len(KINDS)] if KINDS[k % len(KINDS)] not in VARIANT_OF else "window") for k, c in enumerate(wide)]
    for ragged in (True, False):
        got, _ = run_gpu(nvs, "records", g, (ragged,))
        assert got == M.records(wide, ragged)


def test_gpu_findall_record_reaches_three_batches(nvs):
    """findall("a") on "a " * k makes 130 columns; the record form gives every row its k matches back"""
    rows = AC.findall_rows(0)
    c = column(nvs, rows)
    assert len(c.findall("a")) == max(AC.FINDALL_KS) > 2 * AC.RECORD_BATCH
    flat, lst = c.findall_record("a", flat=True)
    want = [0 if r is None else r.count(b"a") for r in rows]
    assert np.diff(lst).tolist() == want and host(flat) == [b"a"] * sum(want)
    assert (flat.size(), flat.null_count(), flat.byte_count()) == (sum(want), 0, sum(want))


def test_gpu_cat_takes_16_columns_and_no_more(nvs):
    rows = AC.cat_columns(M.CAT_MAX_COLUMNS + 1, 10)
    cols = [column(nvs, c) for c in rows]
    assert host(cols[0].cat(cols[1:M.CAT_MAX_COLUMNS], b"", b"")) == M.cat(rows[:M.CAT_MAX_COLUMNS], b"", b"")
    with pytest.raises(ValueError):
        cols[0].cat(cols[1:], b"", b"")
    assert host(cols[0].cat(cols[1:2], b"", b"")) == M.cat(rows[:2], b"", b"")  # the column still serves


@pytest.mark.parametrize("name,pos", AC.bad_gather_lists())
def test_gpu_gather_bad_position_in_any_lane(nvs, name, pos):
    rows = AC.rows_of(AC.KBLOCK + 1)
    c = column(nvs, rows)
    with pytest.raises(IndexError):
        c.gather(pos)
    good = [p if 0 <= p < len(rows) else 0 for p in pos]
    assert host(c.gather(good)) == M.gather(rows, good)


def test_gpu_empty_columns(nvs):
    """no rows at all: every op gives an empty column (join: one empty string), none faults"""
    e = column(nvs, [])
    assert host(e.gather([])) == host(e.sublist(0, 5, 2)) == host(e.cat([column(nvs, [])], b":", b"_")) == []
    assert host(e.cat(None, b",", None)) == [b""] and host(e.partition(b" ", flat=True)) == []
    assert host(e.scalar_scatter(b"x", [0], 1)) == [] and host(e.sort(3)) == []
    flat, lst = e.split_record(b" ", -1, flat=True)
    assert host(flat) == [] and lst.tolist() == [0]


# ---- chains ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AC.chains()))
def test_gpu_chain(nvs, oracle_engine, name):
    """The library and the model side by side, compared after every step -- and with them the size, null count and byte
    count the result column states about itself, which the next op relies on."""
    first, steps = AC.chains()[name]
    cur, g = first, column(nvs, first)
    for k, step in enumerate(steps):
        op, extra, args = step(cur)
        want = AC.run_model((name, op, [cur] + extra, args), oracle_engine)
        got, g = run_gpu(nvs, op, [g] + [column(nvs, c) for c in extra], args)
        assert got == want, (name, k, op)
        cur = AC.next_column(want)
        assert (g.size(), g.null_count(), g.byte_count()) == M.metadata(cur), (name, k, op, "metadata")
