"""The case tables of tests/test_gpu_arrays.py, and the model / reference sides of every case.

A case is (id, op, cols, args): `cols` are the input columns as lists of bytes / None, `args` the op's other arguments.
test_arrays_cpu.py runs every case through run_model and run_reference and wants them equal; test_gpu_arrays.py runs
the library on the same cases and wants run_model's answer.  Results are plain values: a column is a list of bytes / None, a
record result is (flat column, list offsets), `order` is a list of ints, an exception is the string "raises".
"""
import itertools
import os
import re

import arrays_model as M
from cpulibs import Col
# RECORD_ROWS is imported, not copied: the issue's rows for the split-record ops are "the existing RECORD_ROWS plus ...", and a
# copy would drift from them.  test_gpu_round2 is a GPU test module, but importing it touches no GPU: it needs numpy, pytest
# and fuzzdata (plain Python) only, all of which the CPU tests have.
from test_gpu_round2 import RECORD_ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kblock():
    """rows per workgroup of the row-parallel kernels, from the library's headers"""
    src = os.path.join(ROOT, "custrings_amd", "csrc")
    for name in ("cs_internal.h", "device_utils.h"):
        with open(os.path.join(src, name)) as f:
            m = re.search(r"constexpr\s+int\s+kBlock\s*=\s*(\d+)\s*;", f.read())
        if m:
            return int(m.group(1))
    raise AssertionError("kBlock is not in the library's headers")


KBLOCK = _kblock()
ROW_COUNTS = [1, 63, 64, 65, KBLOCK - 1, KBLOCK, KBLOCK + 1, 2 * KBLOCK + 1]
RECORD_BATCH = 64  # RecordCols::kMax
VARIANTS = ["as_is", "no_nulls", "all_null"]  # the logical contents the input column kinds of the GPU file come in


def u(s):
    return None if s is None else s.encode("utf8")


_POOL = [b"", b"a", u("é"), u("😀"), b"ab cd", b"\x00", b"a\x00b", b"\t", b"\n", b"x\ty\nz", b" lead", b"trail ", u("héllo wörld"),
         b"a_b_c", b"\x01\x1f ", b"aa", b"aaaaa", b"a:b", u("é_é"), b"k=v;k2=v2", u("😀é a"), b"_", b" "]


def rows_of(n, salt=0, nulls=(0, 63, 64, -1)):
    """n rows: empty, 1-byte, multi-byte, bytes <= 0x20 (NUL, tab, newline among them), most made distinct by their index,
    one row of about 5000 bytes, null rows at `nulls` (-1: the last row)"""
    rows = []
    for i in range(n):
        base = _POOL[(i * 7 + salt) % len(_POOL)]
        rows.append(base if i % 3 == 0 else base + b"%d" % (i + salt))
    if n >= 3:
        rows[n // 2] = b"".join(b"w%d " % ((i + salt) % 10) for i in range(1667)) + u("é")  # 5003 bytes
    for at in nulls:
        at = n - 1 if at == -1 else at
        if at < n:
            rows[at] = None
    return rows


def variant(rows, name):
    if name == "no_nulls":
        return [b"was null" if r is None else r for r in rows]
    if name == "all_null":
        return [None] * len(rows)
    return list(rows)


SUBLISTS = lambda n: [(0, n, 2), (5, 400, 3), (900, 10, -7), (n, 0, -1), (3, 3, 1), (7, 2, 1), (0, 10 ** 6, 5), (1, n, 1)]


def shape_cases(rows):
    """every op of the family on one column of len(rows) rows (the row counts are the block and bitmask-word edges)"""
    n = len(rows)
    other = rows_of(n, 5, nulls=(1, 62, 65, -1))
    m = min(n, 40)
    src = rows_of(m, 11, nulls=(2,))
    pos = [(i * 13) % n for i in range(m)]
    pos[:4] = [-1, n, n - 1, 0][:m]
    if m > 6:
        pos[6] = pos[5]  # one row named twice
    cases = [
        ("gather_reversed", "gather", [rows], (list(range(n - 1, -1, -1)),)),
        ("gather_one_row_3n_times", "gather", [rows], ([n // 2] * (3 * n),)),
        ("gather_empty_list", "gather", [rows], ([],)),
        ("mask_all_false", "gather_mask", [rows], ([False] * n,)),
        ("mask_all_true", "gather_mask", [rows], ([True] * n,)),
        ("mask_every_third", "gather_mask", [rows], ([i % 3 == 0 for i in range(n)],)),
        ("remove_strings", "remove_strings", [rows], ([0, n - 1, 2, 2, -1, n],)),
        ("scatter", "scatter", [rows, src], (pos,)),
        ("scalar_scatter", "scalar_scatter", [rows], (u("é+"), pos)),
        ("scalar_scatter_null", "scalar_scatter", [rows], (None, pos[: max(1, m // 2)])),
        ("cat_sep", "cat", [rows, other], (b":", None)),
        ("cat_narep", "cat", [rows, other], (None, b"_")),
        ("join", "join", [rows], (b",", None)),
        ("join_narep", "join", [rows], (u("é-"), u("ná"))),
        ("order", "order", [rows], (3, True, True)),
        ("sort_descending", "sort", [rows], (3, False, False)),
        ("records_fixed", "records", [rows, other], (False,)),
        ("records_ragged", "records", [rows, other], (True,)),
    ]
    cases += [("sublist_%d_%d_%d" % t, "sublist", [rows], t) for t in SUBLISTS(n)]
    for d in (b" ", u("é"), b"aa"):
        cases.append(("partition_%r" % d, "partition", [rows], (d,)))
        cases.append(("rpartition_%r" % d, "rpartition", [rows], (d,)))
    for d, k in ((None, -1), (b" ", 2), (b"_", -1), (b"aa", 1)):
        cases.append(("split_record_%r_%d" % (d, k), "split_record", [rows], (d, k)))
        cases.append(("rsplit_record_%r_%d" % (d, k), "rsplit_record", [rows], (d, k)))
    return cases


# ---- records from columns ----------------------------------------------------------------------------------------------
FINDALL_KS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130]


def findall_rows(order):
    """rows "a " * k (k matches of "a"), null and empty rows in between, in two row orders"""
    rows = []
    for k in FINDALL_KS:
        rows += [b"a " * k, None, b""] if k % 2 else [b"a " * k]
    return rows if order == 0 else rows[::-1][3:] + rows[::-1][:3]


WIDE_COLS, WIDE_ROWS = 130, 70


def wide_columns():
    """130 columns of 70 rows.  Rows 1..10 place nulls at the batch edges (row 2: column 63 null and 64 not, row 5: the same
    at 127 / 128, row 8: no null at all, row 10: null everywhere); every later row has one null somewhere else."""
    null_at = {1: [0], 2: [63], 3: [64], 4: [65], 5: [127], 6: [128], 7: [129], 8: [], 9: [63, 64], 10: range(WIDE_COLS), 0: []}
    cols = []
    for c in range(WIDE_COLS):
        col = []
        for r in range(WIDE_ROWS):
            nulls = null_at.get(r, [(r * 7) % WIDE_COLS, (r * 31) % WIDE_COLS])
            if c in nulls:
                col.append(None)
            elif (c + r) % 17 == 0:
                col.append(b"")
            else:
                col.append((u("é%d/") if c % 5 == 0 else b"c%d/") % c + b"r%d" % r)
        cols.append(col)
    return cols


def records_cases():
    wide = wide_columns()
    cases = []
    for ragged in (True, False):
        cases.append(("wide_130_ragged=%d" % ragged, "records", wide, (ragged,)))
        for ncols in (0, 1, 64, 65):
            cases.append(("ncols_%d_ragged=%d" % (ncols, ragged), "records", wide[:ncols], (ragged,)))
        cases.append(("offset_batch_ragged=%d" % ragged, "records", wide[60:], (ragged,)))  # (column 63 is now column 3)
        for order in (0, 1):
            cases.append(("split_columns_order%d_ragged=%d" % (order, ragged), "split_then_records", [findall_rows(order)], (b" ", ragged)))
    for order in (0, 1):
        cases.append(("findall_record_order%d" % order, "findall_record", [findall_rows(order)], ("a",)))
    cases.append(("row_counts_differ", "records", [wide[0], wide[1][:-1]], (True,)))
    return cases


# ---- cat / join ----------------------------------------------------------------------------------------------------------
def cat_columns(ncols, rows=KBLOCK + 1):
    """row 1: null in the first column, row 2: in a middle one, row 3: in the last, row 4: in every column, row 5: all
    empty; later rows have a null now and then"""
    cols = []
    for c in range(ncols):
        col = []
        for r in range(rows):
            null = {1: c == 0, 2: c == ncols // 2, 3: c == ncols - 1, 4: True, 5: False, 0: False}.get(r, (r + 3 * c) % 23 == 0)
            col.append(None if null else b"" if r == 5 else (u("é%d.%d") if r % 4 == 0 else b"%d.%d") % (c, r))
        cols.append(col)
    return cols


SEPS = [None, b"", b":", u("é-")]
NAREPS = [None, b"", b"_", u("ná")]


def cat_cases():
    cases = []
    for nothers in (1, 2, 15):
        cols = cat_columns(nothers + 1)
        for sep, narep in itertools.product(SEPS, NAREPS):
            cases.append(("cat_%d_others_sep=%r_narep=%r" % (nothers, sep, narep), "cat", cols, (sep, narep)))
    cases.append(("cat_row_counts_differ", "cat", [cat_columns(1, 10)[0], cat_columns(1, 9)[0]], (None, None)))
    return cases


def join_rows(n, nulls):
    rows = [(u("jé%d") if r % 2 else b"j%d") % r for r in range(n)]
    at = {"none": [], "first": [0], "last": [n - 1], "run_before_last": list(range(max(0, n - 4), n - 1)), "all": list(range(n))}[nulls]
    for r in at:
        rows[r] = None
    return rows


def join_cases():
    cases = []
    for n in (1, 2, KBLOCK + 1):
        for nulls in ("none", "first", "last", "run_before_last", "all"):
            rows = join_rows(n, nulls)
            for sep, narep in itertools.product((b"", b",", u("é-")), NAREPS):
                cases.append(("join_%d_rows_nulls_%s_sep=%r_narep=%r" % (n, nulls, sep, narep), "join", [rows], (sep, narep)))
    return cases


# ---- scatter / gather ----------------------------------------------------------------------------------------------------
def scatter_cases():
    n = KBLOCK + 1
    rows = rows_of(n)
    src = lambda k: [b"s%d" % j for j in range(k)]
    far = [-1] * (2 * KBLOCK + 10)  # one row named by the first and by the last entry of a list three blocks long
    far[0] = far[-1] = 3
    far[KBLOCK] = 3
    spread = [(j % 5) + 10 for j in range(2 * KBLOCK + 10)]  # five rows, each named a hundred times across three blocks
    long_scalar = b"0123456789" * 600
    some_null = src(6)
    some_null[1] = some_null[4] = None
    cases = [
        ("row_named_twice", "scatter", [rows, src(2)], ([5, 5],)),
        ("row_named_64_times", "scatter", [rows, src(64)], ([7] * 64,)),
        ("row_named_in_three_blocks", "scatter", [rows, src(len(far))], (far,)),
        ("rows_named_100_times", "scatter", [rows, src(len(spread))], (spread,)),
        ("edge_positions", "scatter", [rows, src(4)], ([-1, n, n - 1, 0],)),
        ("no_positions", "scatter", [rows, []], ([],)),
        ("null_sources", "scatter", [rows, some_null], ([9, 10, 11, 10, 12, 12],)),
        ("null_into_column_without_bitmask", "scatter", [variant(rows, "no_nulls"), [None, b"x"]], ([2, n - 1],)),
        ("scalar_row_named_64_times", "scalar_scatter", [rows], (b"S", [7] * 64)),
        ("scalar_edge_positions", "scalar_scatter", [rows], (u("é"), [-1, n, n - 1, 0])),
        ("scalar_no_positions", "scalar_scatter", [rows], (b"S", [])),
        ("scalar_null", "scalar_scatter", [rows], (None, [1, 2, n - 1])),
        ("scalar_null_into_column_without_bitmask", "scalar_scatter", [variant(rows, "no_nulls")], (None, [0, 64])),
        ("scalar_longer_than_any_row", "scalar_scatter", [rows], (long_scalar, [0, 5, 5, n - 1])),
        ("scalar_empty_string", "scalar_scatter", [rows], (b"", [0, 1, 2])),
    ]
    return cases


def bad_gather_lists():
    """one bad position at lane 0, at lane 63, as the last element of a list of kBlock + 1, and alone"""
    n = KBLOCK + 1
    return [("lane_0", [n] + [1] * 63), ("lane_63", [1] * 63 + [-1]), ("last_of_kblock_plus_1", [2] * KBLOCK + [n]), ("alone", [n]),
            ("alone_negative", [-1])]


def gather_cases():
    rows = rows_of(KBLOCK + 1)
    return [("bad_position_" + name, "gather", [rows], (pos,)) for name, pos in bad_gather_lists()]


# ---- split_record / rsplit_record / partition ---------------------------------------------------------------------------
DELIMS = [None, b"", b" ", b"_", u("é"), u("éé"), u("é_"), b"aa"]
LIMITS = [-1, 0, 1, 2, 3, 70]


def token_rows():
    rows = [u(r) for r in RECORD_ROWS]
    rows += [b" ".join(b"t%d" % i for i in range(100)), b"_".join(b"t%d" % i for i in range(200)),
             u("é").join(b"t%d" % i for i in range(100)), u("é_").join(u("tü%d") % i for i in range(100)),
             u("éé").join(b"%d" % i for i in range(75)), b"aa".join(b"b%d" % i for i in range(72))]
    rows += [b" ", b" \t\n" * 21 + b"  ", b"\t", b"\x00 \x00"]  # only whitespace, 1 and 65 bytes; NUL counts as whitespace
    rows += [b"  a b  ", b"__a__b__", u("ééaééébéé"), u("é_é_aé_é_"), u("_é_é"), b"aaXaaaaYaa", b"a b c" + b" " * 30, b" " * 30 + b"a b c"]
    rows += [b"a" * k for k in range(8)]  # "aa" overlaps itself in these
    rows += [d for d in DELIMS if d]  # the delimiter is the whole row
    rows += [b"a", u("é"), b"_", u("é")[:1] + b"x"]  # rows shorter than a delimiter
    rows += [u("x é_y ") * 625 + b"end", None]  # 5003 bytes
    return rows


def split_record_cases():
    rows = token_rows()
    return [("%s_%r_%d" % (op, d, k), op, [rows], (d, k)) for op in ("split_record", "rsplit_record") for d in DELIMS for k in LIMITS]


def partition_cases():
    rows = token_rows()
    return [("%s_%r" % (op, d), op, [rows], (d,)) for op in ("partition", "rpartition") for d in DELIMS if d]


# ---- chains --------------------------------------------------------------------------------------------------------------
def chains():
    """name -> (first column, steps); a step is f(current column) -> (op, the op's other columns, args).  The column an op
    returns (the flat column of a record result) is the next step's input."""
    n = KBLOCK + 1
    other = rows_of(n, 5, nulls=(1, 62, 65, -1))
    rev = lambda cur: list(range(len(cur) - 1, -1, -1))
    return {
        "gather_cat_split_gather_join": (rows_of(n), [
            lambda cur: ("gather", [], (rev(cur),)),
            lambda cur: ("cat", [other], (b":", b"_")),
            lambda cur: ("split_record", [], (b":", -1)),
            lambda cur: ("gather", [], (rev(cur),)),
            lambda cur: ("join", [], (u("é"), None)),
        ]),
        "scatter_sublist_partition_sort_findall": (rows_of(n, 3), [
            lambda cur: ("scatter", [[b"a a", None, b"banana", u("aé a")] * 16], ([(7 * j) % 50 for j in range(64)],)),
            lambda cur: ("sublist", [], (0, len(cur), 3)),
            lambda cur: ("partition", [], (b" ",)),
            lambda cur: ("sort", [], (3, True, True)),
            lambda cur: ("findall_record", [], ("a",)),
        ]),
        "records_remove_rsplit_scatter_cat_rpartition": (rows_of(n, 7), [
            lambda cur: ("records", [other], (True,)),
            lambda cur: ("remove_strings", [], ([0, 5, len(cur) - 1, len(cur)],)),
            lambda cur: ("rsplit_record", [], (None, 2)),
            lambda cur: ("scalar_scatter", [], (None, [0, 63, 64, len(cur) - 1])),
            lambda cur: ("cat", [cur[::-1]], (None, None)),
            lambda cur: ("rpartition", [], (u("é"),)),
        ]),
        "all_null_through_cat_join_split": ([None] * (KBLOCK + 1), [
            lambda cur: ("cat", [rows_of(len(cur), 2)], (b"_", b"")),
            lambda cur: ("gather_mask", [], ([i % 2 == 1 for i in range(len(cur))],)),
            lambda cur: ("join", [], (b" ", None)),
            lambda cur: ("split_record", [], (None, 70)),
            lambda cur: ("rpartition", [], (b"_",)),
        ]),
    }


def next_column(result):
    """what a chain hands on: the column, or the flat column of a record result"""
    return result[0] if isinstance(result, tuple) else result


# ---- the two sides -------------------------------------------------------------------------------------------------------
def outcome(f, *a):
    try:
        return f(*a)
    except (ValueError, IndexError):
        return "raises"


def _ws(d):
    return d or None  # an empty delimiter string splits on whitespace, as no delimiter (cs_records.hip: records())


def _oracle_records(orc, fn, rows, d, k):
    flat, lst = fn(Col.from_list(rows), _ws(d), k)
    return flat.to_bytes_list(), lst.tolist()


def _oracle_findall(orc, rows, pat):
    return [c.to_bytes_list() for c in orc.o.findall(Col.from_list(rows), orc._blob(pat))]


def _oracle_split(orc, rows, d):
    return [c.to_bytes_list() for c in orc.o.split(Col.from_list(rows), d, -1)]


def run_model(case, orc):
    """The expectation.  `orc` (an engines.OracleEngine) serves split_record / rsplit_record, whose statement is the
    oracle's, and turns the rows of the two *_then_records ops into columns; the record step itself is the model's."""
    _, op, cols, args = case
    if op == "split_record":
        return _oracle_records(orc, orc.o.split_record, cols[0], *args)
    if op == "rsplit_record":
        return _oracle_records(orc, orc.o.rsplit_record, cols[0], *args)
    if op == "findall_record":
        return M.records(_oracle_findall(orc, cols[0], args[0]), True)
    if op == "split_then_records":
        return M.records(_oracle_split(orc, cols[0], args[0]), args[1])
    if op in ("partition", "rpartition"):
        return M.partition(cols[0], args[0], op == "rpartition")
    if op in ("cat", "records"):
        return outcome(getattr(M, op), cols, *args)
    return outcome(getattr(M, op), *cols, *args)


def run_reference(case, orc):
    """The second opinion: the oracle's restatement of the reference where it has one; for the record step, which it has
    not, the rows taken apart with zip and takewhile, and for the rows of FINDALL_KS the counts they were built from."""
    _, op, cols, args = case
    o = orc.o
    c = [Col.from_list(x) for x in cols]
    col = lambda f, *a: outcome(lambda: f(*a).to_bytes_list())
    if op in ("split_record", "rsplit_record"):
        return run_model(case, orc)  # (that it runs at all is what test_arrays_cpu.py asks of these two)
    if op == "gather":
        return col(o.gather, c[0], args[0]) if args[0] else []
    if op == "gather_mask":
        return col(o.gather, c[0], [i for i, m in enumerate(args[0]) if m]) if any(args[0]) else []
    if op == "remove_strings":
        keep = [i for i in range(len(cols[0])) if i not in args[0]]
        return col(o.gather, c[0], keep) if keep else []
    if op == "sublist":
        return col(o.sublist, c[0], *args)
    if op == "scatter":
        return col(o.scatter, c[0], c[1], args[0])
    if op == "scalar_scatter":
        return col(o.scatter, c[0], args[0], args[1])
    if op == "cat":
        return col(o.cat, c[0], c[1:], *args)
    if op == "join":
        return col(o.join, c[0], *args)
    if op == "order":
        return o.order(c[0], *args).tolist()
    if op == "sort":
        return col(o.sort, c[0], *args)
    if op in ("partition", "rpartition"):
        flat = o.partition(c[0], args[0], op == "rpartition").to_bytes_list()
        return flat, list(range(0, len(flat) + 1, 3))
    if op == "findall_record":
        assert args[0] == "a", "the second opinion on findall_record counts the byte a: it knows no other pattern"
        recs = [None if r is None else [b"a"] * r.count(b"a") for r in cols[0]]
    elif op == "split_then_records" and args[1]:
        flat, lst = _oracle_records(orc, o.split_record, cols[0], args[0], -1)
        return flat, lst
    else:
        if op == "split_then_records":
            cols = _oracle_split(orc, cols[0], args[0])
        if any(len(x) != len(cols[0]) for x in cols):
            return "raises"
        recs = [list(itertools.takewhile(lambda e: e is not None, rec)) if args[-1] else list(rec) for rec in zip(*cols)]
    flat = [e for rec in recs for e in (rec or [])]
    lst = list(itertools.accumulate([0] + [len(rec or []) for rec in recs]))
    return flat, lst


def all_tables():
    """every table but the per-shape one: name -> cases"""
    return {"records": records_cases(), "cat": cat_cases(), "join": join_cases(), "scatter": scatter_cases(), "gather": gather_cases(),
            "split_record": split_record_cases(), "partition": partition_cases()}
