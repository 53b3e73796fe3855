"""The scan route as a table (cs_regex_scan.hip: scan<MODE>): one case per step of the sequence -- pieces, contains by counts,
class runs, stream kernel, put-off rows, row-wise kernels -- and per row of the stream kernel's table (scan_stream_kernel),
for contains_re, match_re and count_re, on the columns of tests/test_gpu_replace_forms.py and two more (`even-90`, `even-62`).  Every case runs with host
results and with device results and asserts the oracle's values, the returned count, that nothing fell back
(cs_fallback_count) and the route the call took (cs_debug_last_route, cleared beforehand).  The routes are the ones the
library took before the host path was cut into named steps: the table pins them."""
import ctypes as C
import random

import numpy as np
import pytest

import cpulibs
import gpuutil
import test_gpu_replace_forms as forms

pytestmark = pytest.mark.gpu

IPV4, GTEST = forms.IPV4, forms.GTEST
WIDE = r"\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3} "  # six live threads: the tagged DFA's wide executor
WIDE_WORDS = r"\w{5,7} "
BIG, BIGGER = r"(\d|\.){9,12}", r"(\d|\.|a|b){10}"  # no tagged DFA: the list simulator's kernels, of up to 64 instructions and beyond
CONTAINS, MATCH, COUNT = "contains_re", "match_re", "count_re"
ALL = (CONTAINS, MATCH, COUNT)


EVEN = {"even-90": (88, 92), "even-62": (60, 64)}


def _column(kind, n):
    """The columns of tests/test_gpu_replace_forms.py, and two of log lines of even length with a null and an empty row, for
    the forms that leave the automaton's tables in memory once a launch would take more than 40 KB of LDS with them and at
    most 40 KB without.  `even-90`, 88-92 bytes: the widest 64-row tile the 96-bit masks take, an in tile of 5888 bytes --
    the chain form (its LDS is the tables + 5 bytes per byte of in tile + 3.4 KB).  `even-62`, 60-64 bytes, an in tile of
    4096: the bit form of the word-boundary pattern, seven bitmaps (tables + 7.5 bytes per byte of in tile + 4.1 KB; on
    `even-90` its launch takes 59 KB, 48 of them beside the tables, and keeps them in LDS)."""
    if kind not in EVEN:
        return forms._column(kind, n)
    lo, hi = EVEN[kind]
    rnd = random.Random(7000 + n + hi)
    rows = []
    for _ in range(n):
        s = forms._line(rnd)
        while len(s) < hi:
            s += " " + forms._line(rnd)
        rows.append(s[: rnd.randrange(lo, hi + 1)])
    rows[1], rows[2] = None, ""
    return rows


_columns = {}


def _col(kind, n):
    """(host column, device column), made once per shape and never changed."""
    if kind not in EVEN:
        return forms._col(kind, n)
    if (kind, n) not in _columns:
        host = cpulibs.Col.from_list(_column(kind, n))
        _columns[(kind, n)] = (host, gpuutil.from_col(host))
    return _columns[(kind, n)]


# (name, ops, pattern, column, rows, switches); a case's id is name-op
_CASES = [
    # the sequence's steps
    ("pieces", (CONTAINS, COUNT), IPV4, "mid", 1100, ()),
    ("pieces-long", (CONTAINS, COUNT), IPV4, "long", 257, ()),
    ("pieces-later", (CONTAINS, COUNT), GTEST, "accents-long", 1100, ()),
    ("by-counts", (CONTAINS,), r"\w+@\w+", "short", 1100, ()),
    ("units-pattern", (CONTAINS,), r"b|ab", "short", 1100, ("CS_NO_BITS_FORM",)),
    ("by-counts-off", (CONTAINS,), r"\w+@\w+", "short", 1100, ("CS_NO_CONTAINS_BY_COUNT",)),
    ("runs", (COUNT,), r"[a-z]+", "mid", 1100, ()),
    ("words-long", (COUNT,), r"\w+", "long", 257, ()),
    ("runs-forced", (COUNT,), r"[aeiou]+", "short", 257, ("CS_CLASS_RUNS_ALWAYS",)),
    ("runs-off", (COUNT,), r"[a-z]+", "mid", 1100, ("CS_NO_CLASS_RUNS", "CS_NO_VIRTUAL_ROWS")),
    # the stream kernel's forms
    ("plain", ALL, IPV4, "short", 1100, ("CS_NO_UNITS",)),
    ("chain-pattern", (CONTAINS, MATCH), IPV4, "short", 1100, ()),
    ("units", (COUNT,), r"b|ab", "short", 1100, ("CS_NO_BITS_FORM",)),
    ("units-accents", (CONTAINS, COUNT), r"b|ab", "accents", 63, ("CS_NO_BITS_FORM", "CS_NO_CONTAINS_BY_COUNT")),
    ("chain", (COUNT,), IPV4, "short", 1100, ()),
    ("chain-dense", (COUNT,), IPV4, "dense", 1100, ()),  # (rows of 70-92 bytes: the largest in tile of the table)
    ("chain-tables-in-memory", (COUNT,), IPV4, "even-90", 1100, ()),
    ("chain-even-tables-in-lds", (COUNT,), IPV4, "even-90", 1100, ("CS_CHAIN_TABLES_IN_LDS",)),
    ("chain-at", (COUNT,), r"[a-c]+@[a-c]+", "short", 1100, ()),
    ("chain-no-chain-form", (COUNT,), IPV4, "short", 1100, ("CS_NO_CHAIN_FORM",)),
    ("chain-tables-in-lds", (COUNT,), IPV4, "short", 1100, ("CS_CHAIN_TABLES_IN_LDS",)),
    ("bits", (CONTAINS, COUNT), GTEST, "short", 1100, ()),
    ("bits-tables-in-lds", (CONTAINS, COUNT), GTEST, "short", 1100, ("CS_CHAIN_TABLES_IN_LDS",)),
    ("bits-tables-in-memory", (CONTAINS, COUNT), GTEST, "even-62", 1100, ()),
    ("bits-even-tables-in-lds", (CONTAINS, COUNT), GTEST, "even-62", 1100, ("CS_CHAIN_TABLES_IN_LDS",)),
    ("bits-widest-tile", (CONTAINS, COUNT), GTEST, "even-90", 1100, ()),
    ("words", (CONTAINS, COUNT), r"\w+", "short", 1100, ()),
    ("wide", ALL, WIDE, "short", 1100, ()),
    ("wide-words", (CONTAINS, COUNT), WIDE_WORDS, "short", 1100, ()),
    ("wide-long-tile", ALL, WIDE, "mid", 257, ("CS_NO_VIRTUAL_ROWS",)),
    ("plain-later", (CONTAINS,), IPV4, "accents", 1100, ()),
    ("units-later", (CONTAINS, COUNT), r"b|ab", "accents", 1100, ("CS_NO_BITS_FORM", "CS_NO_CONTAINS_BY_COUNT")),
    ("chain-later", (COUNT,), IPV4, "accents", 1100, ()),
    ("bits-later", (CONTAINS, COUNT), GTEST, "accents", 1100, ()),
    ("long-tile", ALL, IPV4, "mid", 1100, ("CS_NO_VIRTUAL_ROWS",)),
    ("long-tile-match", (MATCH,), IPV4, "mid", 1100, ()),
    ("outlier", ALL, IPV4, "outlier", 1100, ()),
    ("outlier-rows", ALL, IPV4, "outlier", 1100, ("CS_NO_VIRTUAL_ROWS",)),
    # the row-wise kernels
    ("rowwise", ALL, IPV4, "short", 1100, ("CS_REGEX_ROWWISE",)),
    ("rowwise-long", ALL, IPV4, "long", 257, ("CS_REGEX_ROWWISE", "CS_NO_VIRTUAL_ROWS")),
    ("rowwise-wide", ALL, WIDE, "short", 257, ("CS_REGEX_ROWWISE",)),
    ("too-large", ALL, BIG, "short", 1100, ()),
    ("too-large-long", ALL, BIG, "long", 65, ()),
    ("larger", ALL, BIGGER, "short", 257, ()),
]
# the chain pattern on every shape: 1, 63, 64, 65, 257 and 1100 rows of each length class
_CASES += [("shape-%s-%d" % (kind, n), ops, IPV4, kind, n, ()) for kind, ops in (("short", ALL), ("mid", (CONTAINS, COUNT)), ("long", (COUNT,))) for n in (1, 63, 64, 65, 257, 1100)]
CASES = [(name + "-" + op, op, pat, kind, n, switches) for name, ops, pat, kind, n, switches in _CASES for op in ops]

ROUTES = {
    'pieces-contains_re': 'pieces:plain',
    'pieces-count_re': 'pieces:chain',
    'pieces-long-contains_re': 'pieces:plain',
    'pieces-long-count_re': 'pieces:chain',
    'pieces-later-contains_re': 'pieces:bits+later',
    'pieces-later-count_re': 'pieces:bits+later',
    'by-counts-contains_re': 'units',
    'units-pattern-contains_re': 'plain',
    'by-counts-off-contains_re': 'plain',
    'runs-count_re': 'runs',
    'words-long-count_re': 'pieces:bits',
    'runs-forced-count_re': 'runs',
    'runs-off-count_re': 'plain',
    'plain-contains_re': 'plain',
    'plain-match_re': 'plain',
    'plain-count_re': 'plain',
    'chain-pattern-contains_re': 'plain',
    'chain-pattern-match_re': 'plain',
    'units-count_re': 'units',
    'units-accents-contains_re': 'units',
    'units-accents-count_re': 'units',
    'chain-count_re': 'chain',
    'chain-dense-count_re': 'chain',
    'chain-tables-in-memory-count_re': 'chain',
    'chain-even-tables-in-lds-count_re': 'chain',
    'bits-tables-in-memory-contains_re': 'bits',
    'bits-tables-in-memory-count_re': 'bits',
    'bits-even-tables-in-lds-contains_re': 'bits',
    'bits-even-tables-in-lds-count_re': 'bits',
    'bits-widest-tile-contains_re': 'bits',
    'bits-widest-tile-count_re': 'bits',
    'chain-at-count_re': 'chain',
    'chain-no-chain-form-count_re': 'units',
    'chain-tables-in-lds-count_re': 'chain',
    'bits-contains_re': 'bits',
    'bits-count_re': 'bits',
    'bits-tables-in-lds-contains_re': 'bits',
    'bits-tables-in-lds-count_re': 'bits',
    'words-contains_re': 'plain',
    'words-count_re': 'bits',
    'wide-contains_re': 'wide',
    'wide-match_re': 'wide',
    'wide-count_re': 'wide',
    'wide-words-contains_re': 'wide',
    'wide-words-count_re': 'wide',
    'wide-long-tile-contains_re': 'wide',
    'wide-long-tile-match_re': 'wide',
    'wide-long-tile-count_re': 'wide',
    'plain-later-contains_re': 'plain+later',
    'units-later-contains_re': 'plain+later',
    'units-later-count_re': 'units+later',
    'chain-later-count_re': 'chain+later',
    'bits-later-contains_re': 'bits+later',
    'bits-later-count_re': 'bits+later',
    'long-tile-contains_re': 'plain',
    'long-tile-match_re': 'plain',
    'long-tile-count_re': 'plain',
    'long-tile-match-match_re': 'plain',
    'outlier-contains_re': 'pieces:plain',
    'outlier-match_re': '',
    'outlier-count_re': 'pieces:chain',
    'rowwise-contains_re': '',
    'rowwise-match_re': '',
    'rowwise-count_re': '',
    'rowwise-long-contains_re': '',
    'rowwise-long-match_re': '',
    'rowwise-long-count_re': '',
    'rowwise-wide-contains_re': '',
    'rowwise-wide-match_re': '',
    'rowwise-wide-count_re': '',
    'too-large-contains_re': '',
    'too-large-match_re': '',
    'too-large-count_re': '',
    'too-large-long-contains_re': '',
    'too-large-long-match_re': '',
    'too-large-long-count_re': '',
    'larger-contains_re': '',
    'larger-match_re': '',
    'larger-count_re': '',
    "outlier-rows-contains_re": "",
    "outlier-rows-match_re": "",
    "outlier-rows-count_re": "",
    **{"shape-short-%d-%s" % (n, op): "chain" if op == COUNT else "plain" for n in (1, 63, 64, 65, 257, 1100) for op in ALL},
    **{"shape-mid-%d-%s" % (n, op): "pieces:chain" if op == COUNT else "pieces:plain" for n in (1, 63, 64, 65, 257, 1100) for op in (CONTAINS, COUNT)},
    **{"shape-long-%d-count_re" % n: "pieces:chain" for n in (1, 63, 64, 65, 257, 1100)},
}

_oracle = None
_wanted = {}


def want(op, pat, kind, n):
    """The oracle's (values, count) of a case, computed once."""
    global _oracle
    if _oracle is None:
        _oracle = cpulibs.Oracle()
    key = (op, pat, kind, n)
    if key not in _wanted:
        host = cpulibs.Col.from_list(_column(kind, n))
        blob = forms._blob(pat)
        _wanted[key] = _oracle.count_re(host, blob) if op == COUNT else _oracle.contains_re(host, blob, 1 if op == MATCH else 0)
    return _wanted[key]


def call(L, op, g, re, devptr):
    """(values, returned count) of one call: to a host array, or -- `devptr` -- to device memory."""
    fn = getattr(L.lib, "cs_" + op)
    rows = g.size()
    found = C.c_int64(-5)
    if not devptr:
        res = np.full(rows, 7, dtype=np.int32 if op == COUNT else np.uint8)
        L.check(fn(g.m_cptr, re, res.ctypes.data, 0, None, C.byref(found)))
        return res, found.value
    import torch

    t = torch.full((rows,), 7, dtype=torch.int32 if op == COUNT else torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.check(fn(g.m_cptr, re, C.c_void_p(t.data_ptr()), 1, None, C.byref(found)))
    torch.cuda.synchronize()
    return t.cpu().numpy(), found.value


@pytest.mark.parametrize("devptr", [False, True], ids=["host", "devptr"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_scan_form(case, devptr):
    name, op, pat, kind, n, switches = case
    L = gpuutil.lib()
    exp, nexp = want(op, pat, kind, n)
    g = _col(kind, n)[1]
    re = gpuutil.compile_re(pat)
    forms._clear_route(L)
    f0 = int(L.lib.cs_fallback_count())
    for v in switches:
        L.check(L.lib.cs_config_set(v.encode(), b"1"))
    try:
        got, ngot = call(L, op, g, re, devptr)
        route = L.lib.cs_debug_last_route().decode()
    finally:
        for v in switches:
            L.check(L.lib.cs_config_set(v.encode(), None))
        L.lib.cs_regex_destroy(re)
    fallbacks = int(L.lib.cs_fallback_count()) - f0
    print("ROUTE %-32s %-20r fallbacks %d" % (name, route, fallbacks))
    assert np.array_equal(got, exp), name
    assert ngot == nexp, (name, ngot, nexp)
    assert fallbacks == 0, (name, fallbacks)
    assert route == ROUTES[name], (name, route)
