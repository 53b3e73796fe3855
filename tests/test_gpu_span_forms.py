"""The span routes as a table (cs_regex.hip: cs_extract, cs_findall, cs_replace_with_backrefs): one case per step of each
sequence -- stream kernel (chain form, tables in memory, plain, long tile; packed spans or begins / lens), row-wise kernels
(tagged DFA with the groups, DFA + list simulator, list simulator of up to 64 instructions and beyond), findall's
provisional and exact pass and its counting path, the backrefs two-pass form on the stream kernel and row-wise -- on the
columns of tests/test_gpu_replace_forms.py and the `even-90` column of tests/test_gpu_scan_forms.py.  Every case asserts
the oracle's columns bit for bit and their number, the offset width of every output column (the packed tail writes 32-bit
offsets below 2^31 bytes, 64-bit ones under CS_SPANS_OFF64), what cs_fallback_count moved by and the route note the call
left (cs_debug_last_route, cleared beforehand: these ops note nothing of their own, findall's counting path leaves
count_re's).  The figures are the ones the library gave before the host paths were cut into named steps: the table pins
them."""
import ctypes as C

import pytest

import cpulibs
import gpuutil
import test_gpu_replace_forms as forms
import test_gpu_scan_forms as scans

pytestmark = pytest.mark.gpu

IPV4, GTEST, WIDE = forms.IPV4, forms.GTEST, scans.WIDE
EXTRACT, FINDALL, BREFS = "extract", "findall", "replace_with_backrefs"
G3 = r"(\d+)\.(\d+)\.\d+\.(\d+) "  # three groups, each a run of a chain item: the chain form
G5 = r"(\d+)\.(\d+)\.(\d+)\.(\d+)( )"  # more than four groups: no chain form; the backrefs single pass declines
GBIG, GBIGGER = r"((\d|\.){9,12})", r"((\d|\.|a|b){10})"  # no tagged DFA: the list simulator, up to 64 instructions and beyond
GWIDE = r"(\d{1,3})\.\d{1,3}\.\d{1,3}\.\d{1,3} "  # six live threads: no tagged DFA with four
SIZES = (1, 63, 64, 65, 257, 1100)
FAR = "x" * 256 + r"\1"  # a reference at a position beyond 255: the template does not pack

# (name, op, pattern, template, column, rows, switches)
CASES = [
    # extract
    ("x-chain", EXTRACT, G3, None, "short", 1100, ()),
    ("x-chain-tables-in-lds", EXTRACT, G3, None, "short", 1100, ("CS_CHAIN_TABLES_IN_LDS",)),
    ("x-no-chain-form", EXTRACT, G3, None, "short", 1100, ("CS_NO_CHAIN_FORM",)),
    ("x-accents", EXTRACT, G3, None, "accents", 1100, ()),
    ("x-five-groups", EXTRACT, G5, None, "short", 1100, ()),
    ("x-unpacked", EXTRACT, G3, None, "short", 1100, ("CS_SPANS_UNPACKED",)),
    ("x-unpacked-rowwise-write", EXTRACT, G3, None, "short", 1100, ("CS_SPANS_UNPACKED", "CS_SPANS_ROWWISE")),
    ("x-off64", EXTRACT, G3, None, "short", 1100, ("CS_SPANS_OFF64",)),
    ("x-mid", EXTRACT, G3, None, "mid", 1100, ()),
    ("x-long", EXTRACT, G3, None, "long", 257, ()),
    ("x-outlier", EXTRACT, G3, None, "outlier", 1100, ()),
    ("x-rowwise", EXTRACT, G3, None, "short", 1100, ("CS_REGEX_ROWWISE",)),
    ("x-lists", EXTRACT, G3, None, "short", 1100, ("CS_EXTRACT_LISTS",)),
    ("x-no-tdfa", EXTRACT, G3, None, "short", 1100, ("CS_REGEX_NO_TDFA",)),
    ("x-big", EXTRACT, GBIG, None, "short", 1100, ()),
    ("x-bigger", EXTRACT, GBIGGER, None, "short", 257, ()),
    ("x-wide", EXTRACT, GWIDE, None, "short", 1100, ()),
    ("x-no-groups", EXTRACT, IPV4, None, "short", 257, ()),
    # findall
    ("f-chain", FINDALL, IPV4, None, "short", 1100, ()),
    ("f-tables-in-memory", FINDALL, IPV4, None, "even-90", 1100, ()),
    ("f-even-tables-in-lds", FINDALL, IPV4, None, "even-90", 1100, ("CS_CHAIN_TABLES_IN_LDS",)),
    ("f-no-chain-form", FINDALL, IPV4, None, "short", 1100, ("CS_NO_CHAIN_FORM",)),
    ("f-no-units", FINDALL, IPV4, None, "short", 1100, ("CS_NO_UNITS",)),
    ("f-units", FINDALL, r"b|ab", None, "short", 1100, ()),
    ("f-gtest", FINDALL, GTEST, None, "short", 1100, ()),
    ("f-exact-pass", FINDALL, r"\d+", None, "short", 1100, ()),
    ("f-exact-unpacked", FINDALL, r"\d+", None, "short", 1100, ("CS_SPANS_EXACT_UNPACKED",)),
    ("f-unpacked", FINDALL, r"\d+", None, "short", 1100, ("CS_SPANS_UNPACKED",)),
    ("f-exact-31-columns", FINDALL, r"[a-z]", None, "short", 257, ()),
    # (more columns than one round of the write kernel takes: `short` rows hold at most 32 letters, `even-90` rows more)
    ("f-many-columns", FINDALL, r"[a-z]", None, "even-90", 257, ()),
    ("f-mid", FINDALL, IPV4, None, "mid", 1100, ()),
    ("f-outlier", FINDALL, IPV4, None, "outlier", 1100, ()),
    ("f-rowwise", FINDALL, IPV4, None, "short", 1100, ("CS_REGEX_ROWWISE",)),
    ("f-no-tdfa", FINDALL, IPV4, None, "short", 1100, ("CS_REGEX_NO_TDFA",)),
    ("f-big", FINDALL, scans.BIG, None, "short", 1100, ()),
    ("f-bigger", FINDALL, scans.BIGGER, None, "short", 257, ()),
    ("f-nowhere", FINDALL, r"zzz", None, "short", 257, ()),
    # replace_with_backrefs, the two-pass form
    ("b-two-pass", BREFS, G3, r"\3.\2.\1 ", "short", 1100, ("CS_BACKREFS_TWO_PASS",)),
    ("b-two-pass-mid", BREFS, G3, r"\3.\2.\1 ", "mid", 1100, ("CS_BACKREFS_TWO_PASS",)),
    ("b-outlier", BREFS, G3, r"\3.\2.\1 ", "outlier", 1100, ("CS_BACKREFS_TWO_PASS",)),
    ("b-rowwise", BREFS, G3, r"\3.\2.\1 ", "short", 1100, ("CS_BACKREFS_TWO_PASS", "CS_REGEX_ROWWISE")),
    ("b-five-groups", BREFS, G5, r"\4.\3.\2.\1\5", "short", 1100, ()),
    ("b-alternation", BREFS, r"(GET|POST) (\S+)", r"\2 \1", "short", 1100, ()),
    ("b-no-groups", BREFS, IPV4, "<IP>", "short", 1100, ()),
    ("b-far-reference", BREFS, r"(\d+)\.", FAR, "short", 257, ()),
    ("b-no-tdfa", BREFS, G3, r"\3.\2.\1 ", "short", 1100, ("CS_REGEX_NO_TDFA",)),
    ("b-big", BREFS, GBIG, r"<\1>", "short", 1100, ()),
    ("b-bigger", BREFS, GBIGGER, r"<\1>", "short", 257, ()),
]
CASES += [("x-shape-%d" % n, EXTRACT, G3, None, "short", n, ()) for n in SIZES]
CASES += [("f-shape-%d" % n, FINDALL, IPV4, None, "short", n, ()) for n in SIZES]
CASES += [("b-shape-%d" % n, BREFS, G3, r"\3.\2.\1 ", "short", n, ("CS_BACKREFS_TWO_PASS",)) for n in SIZES]

# name -> (route note, the offset widths of the output columns, what cs_fallback_count moved by).  Width 4: the packed
# tail's 32-bit offsets; 8: the packed tail under CS_SPANS_OFF64 and the columns built from lengths.  The note is '' but
# where findall's counting path (count_re: scan<2>) left its own, on the `outlier` column's pieces; with CS_REGEX_ROWWISE
# that path notes ''.  The backrefs cases that fall from the single pass to the two-pass form (five groups, the
# alternation, the template that does not pack) count no fallback: the single pass declines them before it launches.
PACKED, BUILT = ("", [4], 0), ("", [8], 0)
EXPECT = {
    "x-chain": PACKED,
    "x-chain-tables-in-lds": PACKED,
    "x-no-chain-form": PACKED,
    "x-accents": PACKED,
    "x-five-groups": PACKED,
    "x-unpacked": BUILT,
    "x-unpacked-rowwise-write": BUILT,
    "x-off64": BUILT,
    "x-mid": BUILT,
    "x-long": BUILT,
    "x-outlier": BUILT,
    "x-rowwise": BUILT,
    "x-lists": BUILT,
    "x-no-tdfa": BUILT,
    "x-big": BUILT,
    "x-bigger": BUILT,
    "x-wide": BUILT,
    "x-no-groups": ("", [], 0),
    "f-chain": PACKED,
    "f-tables-in-memory": PACKED,
    "f-even-tables-in-lds": PACKED,
    "f-no-chain-form": PACKED,
    "f-no-units": PACKED,
    "f-units": PACKED,
    "f-gtest": PACKED,
    "f-exact-pass": PACKED,
    "f-exact-unpacked": BUILT,
    "f-unpacked": BUILT,
    "f-exact-31-columns": PACKED,
    "f-many-columns": BUILT,
    "f-mid": BUILT,
    "f-outlier": ("pieces:chain", [8], 0),
    "f-rowwise": BUILT,
    "f-no-tdfa": BUILT,
    "f-big": BUILT,
    "f-bigger": BUILT,
    "f-nowhere": BUILT,
    "b-two-pass": BUILT,
    "b-two-pass-mid": BUILT,
    "b-outlier": BUILT,
    "b-rowwise": BUILT,
    "b-five-groups": BUILT,
    "b-alternation": BUILT,
    "b-no-groups": BUILT,
    "b-far-reference": BUILT,
    "b-no-tdfa": BUILT,
    "b-big": BUILT,
    "b-bigger": BUILT,
    **{"x-shape-%d" % n: PACKED for n in SIZES},
    **{"f-shape-%d" % n: PACKED for n in SIZES},
    **{"b-shape-%d" % n: BUILT for n in SIZES},
}

_oracle = None
_wanted = {}


def oracle():
    global _oracle
    if _oracle is None:
        _oracle = cpulibs.Oracle()
    return _oracle


def host_col(kind, n):
    return cpulibs.Col.from_list(scans._column(kind, n))


def want(case):
    """The oracle's columns of a case (a list; one column for replace_with_backrefs), computed once."""
    name, op, pat, tmpl, kind, n, _ = case
    key = (op, pat, tmpl, kind, n)
    if key not in _wanted:
        host, blob = host_col(kind, n), forms._blob(pat)
        if op == BREFS:
            _wanted[key] = [oracle().replace_with_backrefs(host, blob, tmpl)]
        else:
            _wanted[key] = getattr(oracle(), op)(host, blob)
    return _wanted[key]


def run(g, op, pat, tmpl):
    if op == BREFS:
        return [g.replace_with_backrefs(pat, tmpl)]
    return getattr(g, op)(pat)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_span_form(case):
    name, op, pat, tmpl, kind, n, switches = case
    L = gpuutil.lib()
    exp = want(case)
    g = scans._col(kind, n)[1]
    forms._clear_route(L)
    f0 = int(L.lib.cs_fallback_count())
    for v in switches:
        L.check(L.lib.cs_config_set(v.encode(), b"1"))
    try:
        got = run(g, op, pat, tmpl)
        route = L.lib.cs_debug_last_route().decode()
    finally:
        for v in switches:
            L.check(L.lib.cs_config_set(v.encode(), None))
    fallbacks = int(L.lib.cs_fallback_count()) - f0
    widths = sorted(set(int(L.lib.cs_column_offset_width(c.m_cptr)) for c in got))
    print("FORM %-28s %r" % (name, (route, widths, fallbacks)))
    assert len(got) == len(exp), (name, len(got), len(exp))
    for k, (a, b) in enumerate(zip(got, exp)):
        gpuutil.assert_same(a, b, "%s column %d" % (name, k))
    assert (route, widths, fallbacks) == EXPECT[name], name


def test_gpu_span_many_columns_is_many():
    """`[a-z]` on the 88-92 byte rows: more columns than one round of the write kernel takes (32), and not thousands."""
    case = [c for c in CASES if c[0] == "f-many-columns"][0]
    assert 32 < len(want(case)) < 300


# ---- refused arguments and empty inputs ------------------------------------------------------------------------------


def _columns_call(L, fn, g, pat):
    """(status, message, number of columns) of cs_extract / cs_findall."""
    re = gpuutil.compile_re(pat)
    arr = C.POINTER(C.c_void_p)()
    ncols = C.c_int(-5)
    try:
        st = getattr(L.lib, fn)(g.m_cptr, re, None, C.byref(arr), C.byref(ncols))
    finally:
        L.lib.cs_regex_destroy(re)
    return st, L.last_error(), ncols.value


def _backrefs_call(L, g, pat, tmpl):
    """(status, message, column or None) of cs_replace_with_backrefs; `tmpl` None is a NULL template."""
    from custrings_amd import nvstrings

    re = gpuutil.compile_re(pat)
    out = C.c_void_p()
    try:
        st = L.lib.cs_replace_with_backrefs(g.m_cptr, re, None if tmpl is None else tmpl.encode(), None, C.byref(out))
    finally:
        L.lib.cs_regex_destroy(re)
    return st, L.last_error(), nvstrings.nvstrings(out.value) if st == 0 else None


def test_gpu_span_extract_refuses_33_groups():
    L = gpuutil.lib()
    st, msg, _ = _columns_call(L, "cs_extract", scans._col("short", 65)[1], "(a)" * 33)
    assert (st, msg) == (L.CS_ERR_RANGE, "extract: more than 32 capture groups")


def test_gpu_span_backrefs_refuses_17_references():
    L = gpuutil.lib()
    st, msg, _ = _backrefs_call(L, scans._col("short", 65)[1], r"(\d+)", r"\1" * 17)
    assert (st, msg) == (L.CS_ERR_RANGE, "replace_with_backrefs: more than 16 references in the template")


def test_gpu_span_backrefs_refuses_empty_match():
    L = gpuutil.lib()
    st, msg, _ = _backrefs_call(L, scans._col("short", 65)[1], r"(\d*)", r"<\1>")
    assert (st, msg) == (L.CS_ERR_INVALID_ARG, "replace_with_backrefs: the pattern matches the empty string")


def test_gpu_span_backrefs_null_template():
    L = gpuutil.lib()
    st, _, got = _backrefs_call(L, scans._col("short", 65)[1], G3, None)
    assert st == 0
    gpuutil.assert_same(got, cpulibs.Col.from_list([None] * 65), "NULL template")


def test_gpu_span_zero_rows():
    L = gpuutil.lib()
    empty = cpulibs.Col.from_list([])
    g = gpuutil.from_col(empty)
    assert _columns_call(L, "cs_extract", g, G3)[::2] == (0, 0)
    assert _columns_call(L, "cs_findall", g, IPV4)[::2] == (0, 0)
    st, _, got = _backrefs_call(L, g, G3, r"\1")
    assert st == 0 and got.size() == 0
    gpuutil.assert_same(got, empty, "zero rows")
