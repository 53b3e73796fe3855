"""The split route as a table (cs_ops.hip: split_impl; cs_split.hip: cs::split_fast): one case per step of the tile plan --
the 92- and 188-byte sentinel walks, the first generation at 64 rows, its sub-tiles of 32 / 16 / 8 rows, the outlier form,
the row-wise kernels -- and per kernel form (whitespace, delimiters of 2..8 bytes, a split limit, rsplit, the measurement
switches, the offset width), on columns of about 1100 rows of at most 188 bytes and 257 longer ones, a null row, an empty
row and a few multi-byte characters in each.  Every case asserts the oracle's columns bit for bit, their count, the
offset width (cs_column_offset_width), that nothing fell back (cs_fallback_count; the single pass's give-up apart) and
the route the call took (cs_debug_last_route, cleared beforehand).  The routes, counts and widths are the ones the
library gave before the host path was cut into named steps: the table pins them, also where a case lands somewhere
unexpected (noted beside it).  The route note does not tell sub-tiles of 32 rows from 16 from 8: the launches do
(tools/replace_launches.py run split; profiles/splitplan)."""
import random

import pytest

import cpulibs
import gpuutil
import test_gpu_replace_forms as forms

pytestmark = pytest.mark.gpu

WORDS = "the in of GET POST index error status ok alice bob id page cab abc k::v baab x--------y p---------q aa".split()
ACCENTS = ("café", "été", "naïve")
D8, D9 = "-" * 8, "-" * 9


def _fit(rnd, size, exact=False):
    """A line of words between single blanks, of at most `size` bytes (`exact`: of `size` bytes); one word in sixteen has
    a two-byte character.  Words have two letters at least: a row of n bytes has at most (n + 1) / 3 tokens.  A line of
    hundreds of bytes says every word size / 100 times over, so that its tokens stay below the 64 columns of the tile
    kernels."""
    w = []
    n = 0
    while n < size + 8:
        w.append((rnd.choice(ACCENTS) if rnd.randrange(16) == 0 else rnd.choice(WORDS)) * max(1, size // 100))
        n += len(w[-1].encode()) + 1
    s = " ".join(w).encode()[:size].decode("utf-8", "ignore").rstrip(" ")
    if exact:
        s += "x" * (size - len(s.encode()))
    return s


def _tokens(n):
    return " ".join("abcdefghij"[i % 10] for i in range(n))


# kind -> (shortest, longest) row in bytes
SIZES = {"s92": (0, 92), "m188": (40, 150), "r200": (190, 210), "r400": (380, 420), "r800": (760, 840), "r1600": (1520, 1680),
         "r4000": (3800, 4200)}


def _column(kind, n):
    base = {"m189": "m188", "outlier": "s92", "c33": "s92", "c65": "m188"}.get(kind, kind)
    if kind == "nulls":
        return [None] * n
    lo, hi = SIZES[base]
    rnd = random.Random(4100 + 7 * n + hi)
    rows = [_fit(rnd, rnd.randrange(lo, hi + 1)) for _ in range(n)]
    for i, v in ((1, None), (2, "")):
        if n > i + 1:
            rows[i] = v
    if base == "m188":  # the longest row the six-word walk takes, and (m189) one byte more
        rows[n // 3] = _fit(rnd, 188, exact=True)
    if kind == "m189":
        rows[n // 2] = _fit(rnd, 189, exact=True)
    if kind == "outlier":  # one row of 10 KB among short ones: no sub-tile size fits the column's largest span
        rows[n // 2] = _fit(rnd, 10 * 1024, exact=True)
    if kind == "c33":  # 33 tokens in 65 bytes: one column more than the three-word walk keeps
        rows[5] = _tokens(33)
    if kind == "c65":  # 65 tokens in 129 bytes: one column more than any tile kernel keeps
        rows[5] = _tokens(65)
    return rows


SPLIT, RSPLIT = "split", "rsplit"
# (name, op, delimiter, maxsplit, column, rows, switches); a switch is NAME or NAME=VALUE
CASES = [
    # the tile plan's steps
    ("walk-92", SPLIT, " ", -1, "s92", 1100, ()),
    ("walk-188", SPLIT, " ", -1, "m188", 1100, ()),
    ("row-of-189", SPLIT, " ", -1, "m189", 1100, ()),
    ("rows-200", SPLIT, " ", -1, "r200", 257, ()),
    ("sub-32", SPLIT, " ", -1, "r400", 257, ()),
    ("sub-16", SPLIT, " ", -1, "r800", 257, ()),
    ("sub-8", SPLIT, " ", -1, "r1600", 257, ()),
    ("no-sub-tile-fits", SPLIT, " ", -1, "r4000", 641, ()),
    # (five sub-tiles: however wide, they count as "a few", and the outlier form takes the column)
    ("no-sub-tile-fits-few-tiles", SPLIT, " ", -1, "r4000", 257, ()),
    ("few-tiles-no-outlier-tiles", SPLIT, " ", -1, "r4000", 257, ("CS_NO_OUTLIER_TILES",)),
    ("outlier", SPLIT, " ", -1, "outlier", 1100, ()),
    # (without sub-tiles these columns of five sub-tiles take the outlier form; without the outlier form the 13 KB span of the
    # outlier column still fits a 64-row tile of the first generation: same route note, other launches)
    ("sub-32-no-small-tiles", SPLIT, " ", -1, "r400", 257, ("CS_NO_SMALL_TILES",)),
    ("sub-8-no-small-tiles", SPLIT, " ", -1, "r1600", 257, ("CS_NO_SMALL_TILES",)),
    ("outlier-no-small-tiles", SPLIT, " ", -1, "outlier", 1100, ("CS_NO_SMALL_TILES",)),
    ("sub-32-no-outlier-tiles", SPLIT, " ", -1, "r400", 257, ("CS_NO_OUTLIER_TILES",)),
    ("outlier-no-outlier-tiles", SPLIT, " ", -1, "outlier", 1100, ("CS_NO_OUTLIER_TILES",)),
    ("outlier-neither", SPLIT, " ", -1, "outlier", 1100, ("CS_NO_SMALL_TILES", "CS_NO_OUTLIER_TILES")),
    # the forms
    ("whitespace", SPLIT, None, -1, "s92", 1100, ()),
    ("whitespace-limit", SPLIT, None, 3, "s92", 1100, ()),
    # (whitespace runs on the 96-bit masks only: a row beyond them sends the call to the row-wise kernels)
    ("whitespace-188", SPLIT, None, -1, "m188", 1100, ()),
    ("two-bytes", SPLIT, "::", -1, "s92", 1100, ()),
    ("eight-bytes", SPLIT, D8, -1, "s92", 1100, ()),
    ("nine-bytes", SPLIT, D9, -1, "s92", 1100, ()),
    ("non-ascii", SPLIT, "é", -1, "s92", 1100, ()),
    ("limit", SPLIT, " ", 3, "s92", 1100, ()),
    ("limit-188", SPLIT, " ", 3, "m188", 1100, ()),
    ("rsplit-limit", RSPLIT, " ", 3, "s92", 1100, ()),
    ("rsplit-limit-rowwise", RSPLIT, " ", 3, "s92", 1100, ("CS_RSPLIT_ROWWISE",)),
    # (rsplit has no first generation: rows of 400 bytes are the row-wise kernels')
    ("rsplit-limit-400", RSPLIT, " ", 3, "r400", 257, ()),
    ("rsplit-no-limit", RSPLIT, " ", -1, "s92", 1100, ()),
    ("rsplit-whitespace", RSPLIT, None, -1, "s92", 1100, ()),
    ("rsplit-whitespace-limit", RSPLIT, None, 3, "s92", 1100, ()),
    ("rsplit-two-bytes", RSPLIT, "::", -1, "s92", 1100, ()),
    ("rsplit-overlapping", RSPLIT, "aa", -1, "s92", 1100, ()),
    ("generic-walk", SPLIT, " ", -1, "s92", 1100, ("CS_SPLIT_GENERIC_WALK",)),
    ("generic-walk-188", SPLIT, " ", -1, "m188", 1100, ("CS_SPLIT_GENERIC_WALK",)),
    ("no-long-walk", SPLIT, " ", -1, "m188", 1100, ("CS_SPLIT_NO_LONG_WALK",)),
    ("no-long-walk-92", SPLIT, " ", -1, "s92", 1100, ("CS_SPLIT_NO_LONG_WALK",)),
    ("old-emit", SPLIT, " ", -1, "s92", 1100, ("CS_SPLIT_OLD_EMIT",)),
    ("old-emit-whitespace", SPLIT, None, -1, "s92", 1100, ("CS_SPLIT_OLD_EMIT",)),
    ("generic", SPLIT, " ", -1, "s92", 1100, ("CS_SPLIT_GENERIC",)),
    ("off64-walk-92", SPLIT, " ", -1, "s92", 1100, ("CS_SPLIT_OFF64",)),
    ("off64-walk-188", SPLIT, " ", -1, "m188", 1100, ("CS_SPLIT_OFF64",)),
    ("off64-general", SPLIT, " ", 3, "s92", 1100, ("CS_SPLIT_OFF64",)),
    ("off64-whitespace", SPLIT, None, -1, "s92", 1100, ("CS_SPLIT_OFF64",)),
    ("off64-two-bytes", SPLIT, "::", -1, "s92", 1100, ("CS_SPLIT_OFF64",)),
    ("off64-first-generation", SPLIT, " ", -1, "r200", 257, ("CS_SPLIT_OFF64",)),
    ("off64-sub-16", SPLIT, " ", -1, "r800", 257, ("CS_SPLIT_OFF64",)),
    ("columns-33", SPLIT, " ", -1, "c33", 1100, ()),
    ("columns-65", SPLIT, " ", -1, "c65", 1100, ()),
    ("nulls-only", SPLIT, " ", -1, "nulls", 257, ()),
    ("nulls-only-whitespace", SPLIT, None, -1, "nulls", 257, ()),
    ("one-row", SPLIT, " ", -1, "s92", 1, ()),
    ("rows-64", SPLIT, " ", -1, "s92", 64, ()),
    ("rows-65", SPLIT, " ", -1, "s92", 65, ()),
    ("rows-65-limit", SPLIT, " ", 3, "s92", 65, ()),
    ("no-rows", SPLIT, " ", -1, "s92", 0, ()),
    ("no-rows-rsplit", RSPLIT, " ", 3, "s92", 0, ()),
]
# the single pass (the experiments build): plain, on the sampled estimate (188 sub-tiles, 169 of them sampled), and giving up
SINGLE = [
    ("single", SPLIT, " ", -1, "s92", 12000, ("CS_SPLIT_SINGLE",)),
    ("single-general", SPLIT, " ", 3, "s92", 12000, ("CS_SPLIT_SINGLE",)),
    ("single-estimate", SPLIT, " ", -1, "s92", 12000, ("CS_SPLIT_SINGLE", "CS_SPLIT1_SAMPLE=169")),
    ("single-gives-up", SPLIT, " ", -1, "s92", 12000, ("CS_SPLIT_SINGLE", "CS_SPLIT1_SHRINK=4")),
]

# name -> (route, columns, offset widths of the columns, fallbacks counted)
EXPECT = {
    'walk-92': ('split-tiles-92', 23, (4,), 0),
    'walk-188': ('split-tiles-188', 36, (4,), 0),
    'row-of-189': ('split-first-generation', 36, (4,), 0),
    'rows-200': ('split-first-generation', 45, (4,), 0),
    'sub-32': ('split-first-generation', 35, (4,), 0),
    'sub-16': ('split-first-generation', 31, (4,), 0),
    'sub-8': ('split-first-generation', 34, (4,), 0),
    'no-sub-tile-fits': ('split-rowwise', 33, (8,), 0),
    'no-sub-tile-fits-few-tiles': ('split-first-generation', 31, (4,), 0),
    'few-tiles-no-outlier-tiles': ('split-rowwise', 31, (8,), 0),
    'outlier': ('split-first-generation', 24, (4,), 0),
    'sub-32-no-small-tiles': ('split-first-generation', 35, (4,), 0),
    'sub-8-no-small-tiles': ('split-first-generation', 34, (4,), 0),
    'outlier-no-small-tiles': ('split-first-generation', 24, (4,), 0),
    'sub-32-no-outlier-tiles': ('split-first-generation', 35, (4,), 0),
    'outlier-no-outlier-tiles': ('split-first-generation', 24, (4,), 0),
    'outlier-neither': ('split-first-generation', 24, (4,), 0),
    'whitespace': ('split-tiles', 23, (4,), 0),
    'whitespace-limit': ('split-tiles', 4, (4,), 0),
    'whitespace-188': ('split-rowwise', 36, (8,), 0),
    'two-bytes': ('split-tiles', 5, (4,), 0),
    'eight-bytes': ('split-tiles', 6, (4,), 0),
    'nine-bytes': ('split-rowwise', 5, (8,), 0),
    'non-ascii': ('split-rowwise', 7, (8,), 0),
    'limit': ('split-tiles', 4, (4,), 0),
    'limit-188': ('split-first-generation', 4, (4,), 0),
    'rsplit-limit': ('split-tiles', 4, (4,), 0),
    'rsplit-limit-rowwise': ('split-rowwise', 4, (8,), 0),
    'rsplit-limit-400': ('split-rowwise', 4, (8,), 0),
    'rsplit-no-limit': ('split-tiles-92', 23, (4,), 0),
    'rsplit-whitespace': ('split-tiles', 23, (4,), 0),
    'rsplit-whitespace-limit': ('split-rowwise', 4, (8,), 0),
    'rsplit-two-bytes': ('split-rowwise', 5, (8,), 0),
    'rsplit-overlapping': ('split-rowwise', 8, (8,), 0),
    'generic-walk': ('split-tiles', 23, (4,), 0),
    'generic-walk-188': ('split-first-generation', 36, (4,), 0),
    'no-long-walk': ('split-first-generation', 36, (4,), 0),
    'no-long-walk-92': ('split-tiles-92', 23, (4,), 0),
    'old-emit': ('split-first-generation', 23, (4,), 0),
    'old-emit-whitespace': ('split-rowwise', 23, (8,), 0),
    'generic': ('split-rowwise', 23, (8,), 0),
    'off64-walk-92': ('split-tiles-92', 23, (8,), 0),
    'off64-walk-188': ('split-tiles-188', 36, (8,), 0),
    'off64-general': ('split-tiles', 4, (8,), 0),
    'off64-whitespace': ('split-tiles', 23, (8,), 0),
    'off64-two-bytes': ('split-tiles', 5, (8,), 0),
    'off64-first-generation': ('split-first-generation', 45, (8,), 0),
    'off64-sub-16': ('split-first-generation', 31, (8,), 0),
    'columns-33': ('split-first-generation', 33, (4,), 0),
    'columns-65': ('split-rowwise', 65, (8,), 0),
    'nulls-only': ('split-rowwise', 1, (8,), 0),
    'nulls-only-whitespace': ('split-rowwise', 1, (8,), 0),
    'one-row': ('split-tiles-92', 16, (4,), 0),
    'rows-64': ('split-tiles-92', 21, (4,), 0),
    'rows-65': ('split-tiles-92', 22, (4,), 0),
    'rows-65-limit': ('split-tiles', 4, (4,), 0),
    'no-rows': ('split-rowwise', 1, (8,), 0),
    'no-rows-rsplit': ('split-rowwise', 1, (8,), 0),
    'single': ('', 23, (4,), 0),
    'single-general': ('', 4, (4,), 0),
    'single-estimate': ('', 23, (4,), 0),
    'single-gives-up': ('split-tiles-92', 23, (4,), 1),
}

_columns = {}
_wanted = {}
_oracle = None


def _col(kind, n):
    """(host column, device column), made once per shape and never changed."""
    if (kind, n) not in _columns:
        host = cpulibs.Col.from_list(_column(kind, n))
        _columns[(kind, n)] = (host, gpuutil.from_col(host))
    return _columns[(kind, n)]


def want(op, delim, maxsplit, kind, n):
    """The oracle's columns of a case, computed once."""
    global _oracle
    if _oracle is None:
        _oracle = cpulibs.Oracle()
    key = (op, delim, maxsplit, kind, n)
    if key not in _wanted:
        _wanted[key] = getattr(_oracle, op)(_col(kind, n)[0], delim, maxsplit)
    return _wanted[key]


def run_case(case):
    """Makes the call and compares its columns with the oracle's; (route, columns, offset widths, fallbacks)."""
    name, op, delim, maxsplit, kind, n, switches = case
    L = gpuutil.lib()
    exp = want(op, delim, maxsplit, kind, n)
    g = _col(kind, n)[1]
    forms._clear_route(L)
    f0 = int(L.lib.cs_fallback_count())
    pairs = [(v.split("=") + ["1"])[:2] for v in switches]
    for k, v in pairs:
        L.check(L.lib.cs_config_set(k.encode(), v.encode()))
    try:
        got = getattr(g, op)(delim, maxsplit)
        route = L.lib.cs_debug_last_route().decode()
    finally:
        for k, _ in pairs:
            L.check(L.lib.cs_config_set(k.encode(), None))
    fallbacks = int(L.lib.cs_fallback_count()) - f0
    widths = tuple(sorted({int(L.lib.cs_column_offset_width(c.m_cptr)) for c in got}))
    assert len(got) == len(exp), (name, len(got), len(exp))
    for k, (a, b) in enumerate(zip(got, exp)):
        gpuutil.assert_same(a, b, "%s column %d" % (name, k))
    return route, len(got), widths, fallbacks


def _check(case):
    seen = run_case(case)
    print("FORM %-28s %r" % (case[0], seen))
    assert seen == EXPECT[case[0]], (case[0], seen)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_split_form(case):
    _check(case)


@pytest.mark.parametrize("case", SINGLE, ids=[c[0] for c in SINGLE])
def test_gpu_split_single_form(case):
    if not gpuutil.lib().lib.cs_has_experiments():
        pytest.skip("the product library is built without the experiments (make exp)")
    _check(case)
