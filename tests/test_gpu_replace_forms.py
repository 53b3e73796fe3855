"""The replace route as a table (cs_regex.hip: cs::replace_re_column): one case per step of the sequence -- pieces, class
runs, single pass, two pass -- and per row of the single pass's kernel table (replace_stream_kernel), on columns of 1 to
about 1100 rows of at most 92, of 94-255 and of more than 255 bytes, a null row and an empty row in each.  Every case
asserts the route the call took (cs_debug_last_route), that no single-pass launch gave up (cs_fallback_count) and the
oracle's column.  The routes are the ones the library took before the host path was cut into named steps: the table
pins them."""
import random

import numpy as np
import pytest

import cpulibs
import engines
import gpuutil

pytestmark = pytest.mark.gpu

IPV4 = r"\d+\.\d+\.\d+\.\d+"
GTEST = r"(\bin\b)|(\ba\b)|(\bthe\b)"
WORDS = "the a in GET POST index error status ok alice bob id page cab abc".split()


def _line(rnd):
    ip = ".".join(str(rnd.randrange(256)) for _ in range(4))
    w = [rnd.choice(WORDS) for _ in range(rnd.randrange(2, 7))]
    return "%s - %s@%s [%d] %s %d" % (ip, rnd.choice("abc") * rnd.randrange(1, 4), rnd.choice("abc"), rnd.randrange(100000), " ".join(w), rnd.randrange(600))


def _rows(kind, n, seed=5):
    """n rows: `short` at most 92 bytes, `mid` 94-255, `long` 260-420; row 1 null and row 2 empty where there are that many."""
    rnd = random.Random(seed * 1000 + n)
    lo, hi = {"short": (20, 92), "mid": (94, 255), "long": (260, 420)}[kind]
    rows = []
    for _ in range(n):
        size = rnd.randrange(lo, hi + 1)
        s = _line(rnd)
        while len(s) < size and kind != "short":
            s += " " + _line(rnd)
        rows.append(s[:size])
    for i, v in ((1, None), (2, "")):
        if n > i + 1:
            rows[i] = v
    return rows


def _column(kind, n):
    if kind == "accents":  # short rows, one in a hundred with a byte >= 0x80: the single pass leaves those rows holes
        rows = _rows("short", n)
        for i in range(7, n, 100):
            rows[i] = "café 10.20.30.40 the été"
        return rows
    if kind == "accents-long":  # ... and rows beyond the 96-bit masks: the pieces' single pass leaves them
        rows = _rows("mid", n)
        for i in range(7, n, 170):
            rows[i] = rows[i][:60] + " café été " + rows[i][60:]
        return rows
    if kind == "outlier":  # one row of about 7000 bytes among short ones: no tile size fits the column's largest span
        rows = _rows("short", n)
        rows[n // 2] = " ".join(_line(random.Random(9)) for _ in range(200))[:7000]
        return rows
    if kind == "dense":  # five matches of `abc` a row: one more than a first attempt is provisioned for; the roomy one holds them
        rnd = random.Random(3)
        rows = ["abc " * 5 + "x" * rnd.randrange(50, 73) for _ in range(n)]
        rows[1], rows[2] = None, ""
        return rows
    return _rows(kind, n)


# (name, op, pattern, replacement, maxrepl, column, rows, switches) -> the route.  The note is cleared before every case
# (_clear_route), so a call that never reaches replace_re_column -- its caller's own kernels note nothing -- leaves ''
RE, LIT, BREFS = "replace_re", "replace", "replace_with_backrefs"
CASES = [
    # the sequence's steps
    ("pieces", RE, IPV4, "<IP>", -1, "mid", 1100, ()),
    ("pieces-bits-holes", RE, r"\w+", "*", -1, "accents-long", 1100, ()),
    ("runs", RE, r"[a-z]+", "*", -1, "mid", 1100, ()),
    ("runs-forced", RE, r"[aeiou]+", "*", -1, "short", 257, ("CS_CLASS_RUNS_ALWAYS",)),
    ("two-pass", RE, IPV4, "<IP>", -1, "short", 1100, ("CS_REGEX_TWO_PASS",)),
    ("two-pass-long", RE, IPV4, "<an-address>", 2, "long", 257, ("CS_REGEX_TWO_PASS",)),
    # the single pass's forms
    ("plain-inplace", RE, IPV4, "<IP>", 1, "short", 1100, ()),
    ("plain-grow", RE, IPV4, "<an-address>", 2, "short", 1100, ()),
    ("plain-long-rows", RE, IPV4, "<IP>", 1, "mid", 1100, ()),
    ("plain-rep16", RE, IPV4, "<an-address>!", 1, "short", 257, ()),
    ("units", RE, r"b|ab", "_", -1, "short", 1100, ("CS_NO_BITS_FORM",)),
    ("units-holes", RE, r"b|ab", "_", -1, "accents", 1100, ("CS_NO_BITS_FORM",)),
    ("bits-holes", RE, r"b|ab", "_", -1, "accents", 1100, ()),
    ("chain-no-chain-form", RE, IPV4, "<IP>", -1, "short", 1100, ("CS_NO_CHAIN_FORM",)),
    ("chain-at", RE, r"[a-c]+@[a-c]+", "<mail>", -1, "short", 1100, ()),
    ("chain", RE, IPV4, "<IP>", -1, "short", 1100, ()),
    ("chain-rep16", RE, IPV4, "<a-longer-one!>", -1, "short", 1100, ()),
    ("chain-tables-in-memory", RE, IPV4, "<IP>", -1, "short", 1100, ("CS_CHAIN_TABLES_IN_MEMORY",)),
    ("chain-holes", RE, IPV4, "<IP>", -1, "accents", 1100, ()),
    ("chain-at-holes", RE, r"[a-c]+@[a-c]+", "<mail>", -1, "accents", 1100, ()),
    ("bits", RE, GTEST, "=", -1, "short", 1100, ()),
    ("bits-tables-in-lds", RE, GTEST, "=", -1, "short", 1100, ("CS_CHAIN_TABLES_IN_LDS",)),
    ("wide", RE, r"\w{5,7} ", "W", -1, "short", 1100, ()),
    ("wide-grow", RE, r"\w{5,7} ", "<a-word> ", -1, "mid", 257, ()),
    ("literal", LIT, "GET", "PUT", -1, "short", 1100, ()),
    ("literal-off", LIT, "GET", "PUT", -1, "short", 1100, ("CS_NO_LITERAL_SCAN",)),
    ("brefs", BREFS, r"(b|ab)c", r"<\1>", -1, "short", 1100, ()),
    ("brefs-chain-at", BREFS, r"([a-c]+)@([a-c]+)", r"\2 at \1", -1, "short", 1100, ()),
    ("brefs-chain", BREFS, r"(\d+)\.(\d+)\.(\d+)\.(\d+)", r"\4.\3.\2.\1", -1, "short", 1100, ()),
    ("brefs-chain-grow", BREFS, r"(\d+)", r"<\1>", -1, "short", 1100, ()),
    # sizing
    ("roomy-retry", RE, r"abc", "abcdefghijklmnop", -1, "dense", 1100, ()),
    ("count-first", RE, r"\d+", "<number>", -1, "short", 1100, ()),
    ("empties", RE, r"x*", "-", -1, "short", 257, ()),
    ("outlier", RE, IPV4, "<IP>", 2, "outlier", 1100, ()),
    ("outlier-grow", RE, IPV4, "<an-address>", 2, "outlier", 1100, ()),
    # the callers with kernels of their own: the single pass declines or is switched off, no fallback is counted
    ("literal-bordered", LIT, "aa", "x", -1, "short", 1100, ("CS_NO_LITERAL_SCAN",)),
    ("literal-long-replacement", LIT, "a", "<a-replacement-of-24-b>", -1, "short", 1100, ()),
    ("replace-own-declined", LIT, " ", "<a-replacement-of-24-b>", -1, "short", 1100, ()),
    ("replace-own-non-plain", LIT, "é", "e", -1, "accents", 1100, ()),
    ("backrefs-own-switch", BREFS, r"(\d+)\.(\d+)", r"\2.\1", -1, "short", 1100, ("CS_BACKREFS_TWO_PASS",)),
    ("backrefs-own-declined", BREFS, r"(\d+)\.(\d+)", r"\2.\1", -1, "mid", 257, ()),
]
# the chain form on every shape: 1, 63, 64, 65, 257 and 1100 rows of each length class
CASES += [("shape-%s-%d" % (kind, n), RE, IPV4, "<IP>", -1, kind, n, ()) for kind in ("short", "mid", "long") for n in (1, 63, 64, 65, 257, 1100)]

ROUTES = {
    'pieces': 'pieces:chain',
    'pieces-bits-holes': 'pieces:bits+later',
    'runs': 'runs',
    'runs-forced': 'runs',
    'two-pass': '',
    'two-pass-long': '',
    'plain-inplace': 'plain',
    'plain-grow': 'plain',
    'plain-long-rows': 'plain',
    'plain-rep16': 'plain',
    'chain': 'chain',
    'chain-rep16': 'chain',
    'chain-tables-in-memory': 'chain',
    'chain-holes': 'chain+later',
    'bits': 'bits',
    'bits-tables-in-lds': 'bits',
    'wide': 'wide',
    'wide-grow': 'wide',
    'literal': 'literal',
    'literal-off': 'plain',
    'brefs': 'brefs',
    'brefs-chain': 'brefs-chain',
    'brefs-chain-grow': 'brefs-chain',
    'roomy-retry': 'chain',
    'count-first': 'chain',
    'empties': 'plain',
    'outlier': 'plain',
    'outlier-grow': 'plain',
    'replace-own-non-plain': '',
    'backrefs-own-switch': '',
    'backrefs-own-declined': '',
    'literal-bordered': 'plain',
    'literal-long-replacement': 'literal',
    'replace-own-declined': '',
    'chain-at': 'chain',
    'chain-at-holes': 'chain+later',
    'units': 'units',
    'units-holes': 'units+later',
    'bits-holes': 'bits+later',
    'brefs-chain-at': 'brefs-chain',
    'chain-no-chain-form': 'chain',
    **{"shape-short-%d" % n: "chain" for n in (1, 63, 64, 65, 257, 1100)},
    **{"shape-%s-%d" % (k, n): "pieces:chain" for k in ("mid", "long") for n in (1, 63, 64, 65, 257, 1100)},
}

_columns = {}
_oracle = None


def _col(kind, n):
    """(host column, device column), made once per shape and never changed."""
    if (kind, n) not in _columns:
        host = cpulibs.Col.from_list(_column(kind, n))
        _columns[(kind, n)] = (host, gpuutil.from_col(host))
    return _columns[(kind, n)]


def _clear_route(L):
    """The thread's route note back to '': a one-row replace_re on the two-pass kernels notes nothing."""
    g = _col("short", 1)[1]
    L.check(L.lib.cs_config_set(b"CS_REGEX_TWO_PASS", b"1"))
    try:
        g.replace("zzz", "y")
    finally:
        L.check(L.lib.cs_config_set(b"CS_REGEX_TWO_PASS", None))
    assert L.lib.cs_debug_last_route() == b""


def _blob(pat):
    b = engines.reference_blob(pat)
    return np.ascontiguousarray(b if b is not None else engines.product_blob(pat), dtype=np.int32)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_replace_form(case):
    global _oracle
    name, op, pat, repl, maxrepl, kind, n, switches = case
    L = gpuutil.lib()
    if _oracle is None:
        _oracle = cpulibs.Oracle()
    host, g = _col(kind, n)
    if op == RE:
        want = _oracle.replace_re(host, _blob(pat), repl, maxrepl)
    elif op == LIT:
        want = _oracle.replace(host, pat, repl, maxrepl)
    else:
        want = _oracle.replace_with_backrefs(host, _blob(pat), repl)
    _clear_route(L)
    f0 = int(L.lib.cs_fallback_count())
    for v in switches:
        L.check(L.lib.cs_config_set(v.encode(), b"1"))
    try:
        if op == RE:
            got = g.replace(pat, repl, maxrepl)
        elif op == LIT:
            got = g.replace(pat, repl, maxrepl, regex=False)
        else:
            got = g.replace_with_backrefs(pat, repl)
        route = L.lib.cs_debug_last_route().decode()
    finally:
        for v in switches:
            L.check(L.lib.cs_config_set(v.encode(), None))
    fallbacks = int(L.lib.cs_fallback_count()) - f0
    print("ROUTE %-28s %-24r fallbacks %d" % (name, route, fallbacks))
    gpuutil.assert_same(got, want, name)
    assert fallbacks == 0, (name, fallbacks)
    assert route == ROUTES[name], (name, route)
