"""split_re / rsplit_re on the MI355X, bit for bit against the model of tests/splitre_model.py (pinned by
tests/test_splitre_cpu.py): row counts around the 64-row tile, largest match counts around findall's provisional width
and around the packed writer's column limit, every limit around a row's match count from both ends, the row contents
that make empty tokens, rows with bytes >= 0x80 and a NUL, a long row among short ones, a column whose tiles do not
fit, the forced routes, the literal against split / rsplit, the record forms, the refusals and the outputs' metadata."""
import ctypes as C

import numpy as np
import pytest

import gpuutil
import splitre_model as m
from cpulibs import Col
from custrings_amd import splitre as S

pytestmark = pytest.mark.gpu

ROUTES = [(), ("CS_SPANS_UNPACKED",), ("CS_REGEX_ROWWISE",), ("CS_REGEX_NO_TDFA",)]


def _L():
    return gpuutil.lib()


class switches:
    def __init__(self, names):
        self.names = names

    def __enter__(self):
        for v in self.names:
            _L().check(_L().lib.cs_config_set(v.encode(), b"1"))

    def __exit__(self, *exc):
        for v in self.names:
            _L().check(_L().lib.cs_config_set(v.encode(), None))


def column(rows):
    _L()
    return gpuutil.from_col(Col.from_list(rows))


def lists(cols):
    return [gpuutil.to_col(c).to_list() for c in cols]


def rows_with(nrows, most):
    """`nrows` rows of very different match counts of ',' (0 .. most, the busiest in the last row), the contents the
    definition names: adjacent matches, a match at either end, a row that is one match, empty and null rows, an é next
    to a delimiter, a NUL"""
    special = ["a,,b", ",lead", "trail,", ",", "", None, "é,é", "x\x00,y", "plain"]
    rows = []
    for i in range(nrows):
        k = (i * 7) % (most + 1)
        rows.append(special[i % len(special)] if i % 3 == 0 and most >= 2 else ",".join("t%d" % j for j in range(k + 1)))
    if nrows:
        rows[-1] = ",".join("é%d" % j for j in range(most + 1)) if most else "none"
    return rows


_cases = {}


def case(nrows, most):
    if (nrows, most) not in _cases:
        _cases[(nrows, most)] = rows_with(nrows, most)
    return _cases[(nrows, most)]


def check(rows, pat, limit, g=None):
    g = g or column(rows)
    assert lists(S.split_re(g, pat, limit)) == m.columns(rows, pat, limit), ("split_re", pat, limit)
    assert lists(S.rsplit_re(g, pat, limit)) == m.columns(rows, pat, limit, reverse=True), ("rsplit_re", pat, limit)


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "+".join(r) or "default")
@pytest.mark.parametrize("nrows", [0, 1, 63, 64, 65, 129])
def test_row_counts(nrows, route):
    rows = case(nrows, 5)
    with switches(route):
        for limit in (-1, 2):
            check(rows, ",", limit)


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "+".join(r) or "default")
@pytest.mark.parametrize("most", [0, 1, 3, 4, 5, 31, 32, 33])
def test_match_counts_and_limits(most, route):
    rows = case(65, most)
    g = column(rows)
    with switches(route):
        for limit in sorted({-1, 0, 1, most - 1, most, most + 1}):
            check(rows, ",", limit, g)
        assert len(S.split_re(g, ",")) == most + 1


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "+".join(r) or "default")
@pytest.mark.parametrize("pat", [r"\s*[,;]\s*", r"\s+", "[,;]+", r"\d+", r" - | \[|\] "])
def test_patterns_and_contents(pat, route):
    rows = ["a, b;c", None, "", ",lead", "trail;", "a,,b", ",", "é , é;x  ;", "nul\x00a , b,c", "one two  three 42 x7y,8",
            "host - - [10/Oct/2000:13:55:36] GET", " ", "7", ("long row, over 93 bytes; " * 5) + "end 12"] * 5
    g = column(rows)
    with switches(route):
        for limit in (-1, 1, 2, 3):
            check(rows, pat, limit, g)


def test_routes():
    """packed spans while the token columns fit one launch of the packed writer (32), begins / lens from the stream kernel
    beyond that and with CS_SPANS_UNPACKED, a thread a row with CS_REGEX_ROWWISE, without the tagged DFA and where the
    tiles do not fit"""
    route = lambda: _L().lib.cs_debug_last_route().decode()
    for most, want in ((5, "splitre-packed"), (31, "splitre-packed"), (32, "splitre-stream"), (33, "splitre-stream")):
        S.split_re(column(case(65, most)), ",")
        assert route() == want, most
    g = column(case(65, 33))
    S.split_re(g, ",", 31)  # (the limit sets the width of both scans)
    assert route() == "splitre-packed"
    S.rsplit_re(g, ",", 31)  # (from the right every match is scanned)
    assert route() == "splitre-stream"
    for sw, want in (("CS_SPANS_UNPACKED", "splitre-stream"), ("CS_REGEX_ROWWISE", "splitre-rowwise"), ("CS_REGEX_NO_TDFA", "splitre-rowwise")):
        with switches((sw,)):
            S.split_re(column(case(65, 5)), ",")
            assert route() == want, sw
    S.split_re(column([("x" * 3000 + ",") * 3, "a,b"] * 40), ",")
    assert route() == "splitre-rowwise"


def test_only_null_rows_and_no_rows_answer_as_split():
    for rows in ([], [None] * 70, ["", None, ""]):
        g = column(rows)
        assert lists(S.split_re(g, ",")) == lists(g.split(",")) == m.columns(rows, ",")
        assert lists(S.rsplit_re(g, ",", 2)) == lists(g.rsplit(",", 2))


def test_tiles_that_do_not_fit_go_row_wise():
    rows = [("x" * 3000 + ",") * 3 + "é", None, "a,b"] * 30  # (a 64-row tile spans some 190 KB)
    check(rows, ",", -1)
    check(rows, "x,", 2)


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "+".join(r) or "default")
def test_literal_is_split_on_the_gpu(route):
    rows = case(129, 5)
    g = column(rows)
    with switches(route):
        assert lists(S.split_re(g, ",")) == lists(g.split(","))
        assert lists(S.rsplit_re(g, ",", 2)) == lists(g.rsplit(",", 2))


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("reverse", [False, True])
def test_record_forms(reverse, on_device):
    import torch

    L = _L()
    rows = case(129, 5)
    g = column(rows)
    for limit in (-1, 2):
        want = m.records(rows, ",", limit, reverse)
        flat_want = [t for r in want if r is not None for t in r]
        loff_want = np.concatenate([[0], np.cumsum([0 if r is None else len(r) for r in want])]).astype(np.int64)
        fn = L.lib.cs_rsplit_record_re if reverse else L.lib.cs_split_record_re
        re = gpuutil.compile_re(",")
        out = C.c_void_p()
        try:
            if on_device:
                dev = torch.full((len(rows) + 3,), -7, dtype=torch.int64, device="cuda")
                L.check(fn(g.m_cptr, re, limit, dev.data_ptr(), 1, None, C.byref(out)))
                torch.cuda.synchronize()
                host = dev.cpu().numpy()
                assert np.all(host[len(rows) + 1:] == -7), "words behind the list offsets were written"
                loff = host[:len(rows) + 1]
            else:
                loff = np.zeros(len(rows) + 1, dtype=np.int64)
                L.check(fn(g.m_cptr, re, limit, loff.ctypes.data, 0, None, C.byref(out)))
        finally:
            L.lib.cs_regex_destroy(re)
        from custrings_amd import nvstrings

        flat = nvstrings.nvstrings(out.value)
        assert np.array_equal(loff, loff_want)
        assert gpuutil.to_col(flat).to_list() == flat_want
    # the Python functions: flat, and one instance a row (None for a null row)
    meth = S.rsplit_record_re if reverse else S.split_record_re
    f, loff = meth(g, ",", 2, flat=True)
    assert np.array_equal(loff, loff_want) and gpuutil.to_col(f).to_list() == flat_want
    per_row = meth(g, ",", 2)
    assert [None if r is None else gpuutil.to_col(r).to_list() for r in per_row] == want


def test_refusals():
    L = _L()
    g = column(["a,b"])
    for pat in ("x*", ""):
        with pytest.raises(ValueError):
            S.split_re(g, pat)
        with pytest.raises(ValueError):
            S.rsplit_re(g, pat, 1)
        with pytest.raises(ValueError):
            S.split_record_re(g, pat)
    re = gpuutil.compile_re(",")
    arr, n, out = C.POINTER(C.c_void_p)(), C.c_int(), C.c_void_p()
    loff = np.zeros(2, dtype=np.int64)
    try:
        for fn in (L.lib.cs_split_re, L.lib.cs_rsplit_re):
            assert fn(g.m_cptr, None, -1, None, C.byref(arr), C.byref(n)) == L.CS_ERR_INVALID_ARG
            assert fn(g.m_cptr, re, -1, None, None, C.byref(n)) == L.CS_ERR_INVALID_ARG
            assert fn(g.m_cptr, re, -1, None, C.byref(arr), None) == L.CS_ERR_INVALID_ARG
            assert fn(None, re, -1, None, C.byref(arr), C.byref(n)) == L.CS_ERR_INVALID_ARG
        for fn in (L.lib.cs_split_record_re, L.lib.cs_rsplit_record_re):
            assert fn(g.m_cptr, None, -1, loff.ctypes.data, 0, None, C.byref(out)) == L.CS_ERR_INVALID_ARG
            assert fn(g.m_cptr, re, -1, loff.ctypes.data, 0, None, None) == L.CS_ERR_INVALID_ARG
            assert fn(g.m_cptr, re, -1, None, 0, None, C.byref(out)) == L.CS_ERR_INVALID_ARG
    finally:
        L.lib.cs_regex_destroy(re)


@pytest.mark.parametrize("route", ROUTES[:3], ids=lambda r: "+".join(r) or "default")
def test_output_metadata(route):
    rows = case(129, 5)
    want = m.columns(rows, ",", 3)
    with switches(route):
        cols = S.split_re(column(rows), ",", 3)
    assert len(cols) == len(want)
    for c, w in zip(cols, want):
        assert c.size() == len(w)
        assert c.len() == [None if t is None else len(t) for t in w]
        assert c.byte_count() == sum(len(t.encode("utf8")) for t in w if t is not None)
    assert gpuutil.to_col(cols[0].upper()).to_list() == [None if t is None else t.upper() for t in want[0]]
