"""Borrowed columns -- from_offsets64(copy=False) over caller memory -- at odd addresses amid hostile bytes.

The pool hands every other column 16-byte aligned buffers with room behind them; a borrowed column has its chars at any
byte address, its int64 offsets at 8 mod 16, and the caller's other data right beside both.  Every op of the matrix in
tests/borrowedutil.py runs on such a column (and, where its family has a switch, on the row-wise route as well) and on
the same bytes through the copying ingest; the answers come from the CPU models and the oracle, computed from the row
list, with no tolerance anywhere.  Results go to caller buffers aligned to their element size only, with canaries on
both sides; the format ops read their values and null masks from such addresses; and a column an op returns must
survive the caller taking its memory back."""
import numpy as np
import pytest

import borrowedutil as bu
import convert_model as cm
import datetime_model as dm

EXPECT = bu.Expect()


# ---- the ASCII poison is consequential (CPU) ---------------------------------------------------------------------------
def test_ascii_poison_changes_every_answer():
    """For every op of the matrix: the CPU answer for the column's first row changes when the 1..15 poison bytes that lie
    in front of it are let into the row, or the answer for its last row changes with the 1..15 bytes behind it -- for every
    one of the fifteen counts.  (is_empty can only change on an empty row: it is held to the first row of the column
    without bytes.)  So a kernel that lets a neighbouring byte into a result fails the GPU tests below."""
    dull = []
    for op in bu.build_ops():
        first, last = (e.encode() for e in bu.ENDS[op.group])
        if op.name == "is_empty":
            first = last = b""
        plain_first, plain_last = op.cpu([first]), op.cpu([last])
        for k in range(1, 16):
            poison = bu.poison_for("ascii", op.group)
            front = op.cpu([bu.poison_front(poison, k) + first])
            behind = op.cpu([last + bu.poison_behind(poison, k)])
            if front == plain_first and behind == plain_last:
                dull.append((op.name, k))
    assert not dull, "the poison changes neither end row's answer for (op, bytes): %s" % dull


def test_builder_lays_the_poison_against_the_column():
    """the byte in front of a column is the poison's last, the byte behind it the poison's first, for every count"""
    for k in (1, 15, 40, 256):
        assert bu.poison_front(bu.ASCII_POISON, k)[-1:] == bu.ASCII_POISON[-1:]
        assert bu.poison_behind(bu.ASCII_POISON, k)[:1] == bu.ASCII_POISON[:1]
        assert len(bu.poison_front(bu.ASCII_POISON, k)) == k == len(bu.poison_behind(bu.ASCII_POISON, k))
    for shape in bu.SHAPES:
        for group in bu.ENDS:
            rows = bu.make_rows(shape, group)
            if shape != "no_bytes":
                assert rows[0] and rows[-1], "the end rows touch the poison"
            else:
                assert not any(rows)


# ---- the matrix on the GPU ---------------------------------------------------------------------------------------------
class Ctx:
    """the other borrowed columns an op takes, placed like the column under test"""

    def __init__(self, rows, shift, offs_mod, poison):
        self.rows, self.shift, self.offs_mod, self.poison = rows, shift, offs_mod, poison
        self.keep = []

    def _col(self, rows):
        b = bu.Borrowed([None if r is None else (r if isinstance(r, bytes) else r.encode()) for r in rows], self.shift, self.offs_mod, self.poison)
        self.keep.append(b)
        return b.col

    def targets(self, M):
        return self._col(bu.TARGETS[M])

    def edit_targets(self):
        return self._col(bu.edit_targets(self.rows))

    def others(self):
        return self._col(self.rows[::-1])


def _first_difference(got, want):
    if isinstance(got, list) and isinstance(want, list):
        if len(got) != len(want):
            return "lengths %d / %d" % (len(got), len(want))
        for i, (a, b) in enumerate(zip(got, want)):
            if a != b:
                return "item %d: %r, the model says %r" % (i, a, b)
    return "%r / %r" % (got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", bu.SHAPES)
@pytest.mark.parametrize("poison", bu.POISONS)
@pytest.mark.parametrize("shift,offs_mod", bu.PLACES)
def test_borrowed_column_matches_the_models(shift, offs_mod, poison, shape, monkeypatch):
    import gpuutil

    gpuutil.lib()
    ops = bu.build_ops()
    failures = []
    for group in bu.ENDS:
        mine = [op for op in ops if op.group == group]
        rows = bu.make_rows(shape, group)
        b = bu.Borrowed(rows, shift, offs_mod, bu.poison_for(poison, group))
        copied = b.copied()
        ctx = Ctx(rows, shift, offs_mod, bu.poison_for(poison, group))
        nulls = sum(r is None for r in rows)
        for name, g in (("borrowed", b.col), ("copied", copied)):
            if g.null_count() != nulls:
                failures.append("null_count of the %s column: %d, the rows hold %d" % (name, g.null_count(), nulls))
            if bu.col_bytes(g) != rows:
                failures.append("the %s column does not export its rows" % name)
        for op in mine:
            want = EXPECT(op, shape)
            for rowwise in ((False, True) if op.switch else (False,)):
                if op.switch:
                    if rowwise:
                        monkeypatch.setenv(op.switch, "1")
                    else:
                        monkeypatch.delenv(op.switch, raising=False)
                got = {"borrowed": op.gpu(b.col, ctx), "copied": op.gpu(copied, ctx)}
                wrong = [k for k in got if got[k] != want]
                if wrong:
                    failures.append("%s (%s): %s differ%s from the model; %s: %s" % (
                        op.name, "row-wise" if rowwise else "default route", " and ".join(wrong), "s" if len(wrong) == 1 else "",
                        wrong[0], _first_difference(got[wrong[0]], want)))
            if op.switch:
                monkeypatch.delenv(op.switch, raising=False)
        if not b.caller_memory_intact():
            failures.append("group %s: the caller's chars or offsets tensor was written to" % group)
    assert not failures, "\n".join(failures)


# ---- format ops: values and null masks read from caller addresses --------------------------------------------------------
FORMAT_N = 1100


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["itos", "ltos", "ftos", "dtos", "int2ip", "from_booleans", "int2timestamp"])
def test_format_ops_read_values_and_nulls_at_element_alignment(op, monkeypatch):
    """values at 4 mod 16 (32-bit), 8 mod 16 (64-bit) or an odd address (bytes), the null mask at an odd address with its
    padding bits set, other data all around: the strings are the models'"""
    from custrings_amd import nvstrings

    import gpuutil

    gpuutil.lib()
    n = FORMAT_N - 3  # (not a multiple of 8: the last mask byte has padding bits)
    rng = np.random.default_rng(11)
    valid_bits = (rng.random(n) > 0.1).astype(np.uint8)
    mask = np.packbits(np.concatenate([valid_bits, np.ones((-n) % 8, dtype=np.uint8)]), bitorder="little")
    if op == "int2timestamp":
        values = dm.gen_values(n, 3)
        want = dm.format_column(values, mask)
    else:
        key = "from_bools" if op == "from_booleans" else op
        values = cm.gen_values(key, n, 3)
        want = cm.format_column(key, values, mask)
    vals = bu.Guarded(values.dtype, n, fill=values)
    nul = bu.Guarded(np.uint8, len(mask), fill=mask)
    for rowwise in (False, True):
        if rowwise:
            monkeypatch.setenv("CS_CONVERT_ROWWISE", "1")
        g = getattr(nvstrings, op)(vals.ptr, count=n, nulls=nul.ptr, bdevmem=True)
        assert bu.col_bytes(g) == want, "%s, %s" % (op, "row-wise" if rowwise else "default route")
        assert g.null_count() == int(n - valid_bits.sum())
    assert np.array_equal(cm.bits(vals.values()), cm.bits(values)) and np.array_equal(nul.values(), mask)


# ---- lifetime: a column an op returns owns what it refers to ---------------------------------------------------------------
def _lifetime_ops():
    from custrings_amd import nvtext

    return {
        "lower": lambda g: g.lower(), "upper": lambda g: g.upper(), "swapcase": lambda g: g.swapcase(),
        "capitalize": lambda g: g.capitalize(), "title": lambda g: g.title(), "wrap": lambda g: g.wrap(10),
        "copy": lambda g: g.copy(), "ngrams_1": lambda g: nvtext.ngrams(g, 1, "_"),
        "sublist_all": lambda g: g.sublist(0, g.size(), 1),
        "replace_tokens_no_targets": lambda g: nvtext.replace_tokens(g, g.sublist(0, 0, 1), ["x"]),
    }


LIFETIME = ["lower", "upper", "swapcase", "capitalize", "title", "wrap", "copy", "ngrams_1", "sublist_all", "replace_tokens_no_targets"]


@pytest.mark.gpu
@pytest.mark.parametrize("rowwise", [False, True], ids=["tiles", "rows"])
@pytest.mark.parametrize("name", LIFETIME)
def test_result_outlives_the_borrowed_column(name, rowwise, monkeypatch):
    """the op's result is read AFTER the borrowed column is gone and the caller has overwritten its tensors in place
    (offsets with zeros -- they describe empty rows, nothing can index out of range --, chars with poison)"""
    import torch

    import gpuutil

    gpuutil.lib()
    rows = bu.make_rows("ragged_tiles", "text")
    if name == "ngrams_1":
        rows = [r if r else b"x" for r in rows]  # (create_ngrams drops null and empty rows: none here, all rows come back)
    ops = {o.name: o for o in bu.build_ops()}
    want = ops[name].cpu(rows) if name in ops else rows
    for switch in ("CS_CASE_ROWWISE", "CS_PAD_ROWWISE"):
        if rowwise:
            monkeypatch.setenv(switch, "1")
    b = bu.Borrowed(rows, 13, 8, bu.ASCII_POISON)
    out = _lifetime_ops()[name](b.col)
    b.col._destroy()
    torch.cuda.synchronize()
    b.offs.zero_()
    b.chars_back.copy_(torch.from_numpy(np.frombuffer(bu.poison_behind(b"\xff", b.chars_back.numel()), dtype=np.uint8).copy()))
    torch.cuda.synchronize()
    got = bu.col_bytes(out)
    assert got == want, "%s reads the caller's memory after the caller took it back: %s" % (name, _first_difference(got, want))
