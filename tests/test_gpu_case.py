"""lower / upper on the MI355X against the oracle and the Python model of tests/case_model.py, with the route proven
(cs_debug_last_route): every BMP character that keeps its UTF-8 width through the tile kernel's table patch (k_case_tile,
cs_case.hip), a width-changing character anywhere handing the whole column to the row kernels, arbitrary bytes that keep
their size through the kernel's malformed branch, the three tile sizes at partial tiles and partial workgroups, tiles beyond
the staging buffer, and borrowed columns whose chars start inside a 16-byte piece.

Every comparison is byte-exact on chars, int64 offsets and validity; the input's digest and the fallback count do not move;
a result of the tile route carries the input's offsets."""
import functools

import numpy as np
import pytest

import borrowedutil as bu
import case_model as cm
import cpulibs
import gpuutil

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    return cpulibs.Oracle()


def _route():
    return gpuutil.lib().lib.cs_debug_last_route().decode()


def _first_difference(got, want, col):
    a, b, src = got.to_bytes_list(), want.to_bytes_list(), col.to_bytes_list()
    for i in range(min(len(a), len(b))):
        if a[i] != b[i]:
            return i, (src[i] or b"")[:96], (a[i] or b"")[:96], (b[i] or b"")[:96]
    return None


def check(op, col, want, route, g=None, model=None):
    """`op` of the device column `g` (default: `col` ingested by copy) against `want` (the oracle's answer) and `model`"""
    L = gpuutil.lib()
    g = g if g is not None else gpuutil.from_col(col)
    before = g.digest()
    f0 = L.lib.cs_fallback_count()
    out = getattr(g, op)()
    took = _route()
    assert took in ("tile", "rows")
    if route is not None:
        assert took == route, (op, took)
    got = gpuutil.to_col(out)  # (_export64)
    for ref in (want, model):
        if ref is None:
            continue
        assert got.rows == ref.rows
        assert np.array_equal(got.bitmask(), ref.bitmask()), (op, "validity")
        if not (np.array_equal(got.offsets, ref.offsets) and np.array_equal(got.chars, ref.chars)):
            raise AssertionError((op, took) + tuple(_first_difference(got, ref, col) or ("offsets",)))
    assert g.digest() == before  # the input is untouched
    assert L.lib.cs_fallback_count() == f0
    if took == "tile":  # the output shares the input's extents
        assert np.array_equal(got.offsets, col.offsets)
    return took


@functools.lru_cache(maxsize=None)
def _well_formed(op, gen):
    """-> (rows, column, the model's answer)"""
    if gen == "with_nulls":
        rows = cm.with_nulls(cm.singles(op)[::3] + cm.embedded(op)[1::3] + cm.packed(op))
    else:
        rows = getattr(cm, gen)(op)
    assert len(rows) < 70_000
    return rows, cpulibs.Col.from_list(rows), cpulibs.Col.from_list(cm.case_column(op, rows))


# ---- 1: every keeper through the tile kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", ["singles", "embedded", "packed", "with_nulls"])
@pytest.mark.parametrize("op", cm.OPS)
def test_every_keeper_through_the_tile_kernel(orc, op, gen):
    """each of the 63,000 BMP characters that keep their width, alone in a row, between ASCII letters, and packed twenty
    to a row with no ASCII between them: all stay on the tile route, mapped through the tables or left as they are"""
    _, col, model = _well_formed(op, gen)
    check(op, col, getattr(orc, op)(col), "tile", model=model)


# ---- 2: a character that changes its width ------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("op", cm.OPS)
def test_one_changer_hands_the_column_to_the_row_kernels(orc, op, where):
    rows = list(_well_formed(op, "embedded")[0])
    change = cm.changers(op)
    at = {"first": 0, "middle": len(rows) // 2 + 11, "last": len(rows) - 1}[where]
    rows[at] = chr(change[at % len(change)])
    col = cpulibs.Col.from_list(rows)
    check(op, col, getattr(orc, op)(col), "rows", model=cpulibs.Col.from_list(cm.case_column(op, rows)))


@pytest.mark.parametrize("op", cm.OPS)
def test_every_changer(orc, op):
    rows = cm.changer_column(op)
    col = cpulibs.Col.from_list(rows)
    check(op, col, getattr(orc, op)(col), "rows", model=cpulibs.Col.from_list(cm.case_column(op, rows)))


# ---- 3: malformed rows that keep their size -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keeping(orc):
    kept, low, up = cm.size_keeping_bytes(7, 40_000, orc)
    return kept, cpulibs.Col.from_list(kept), {"lower": cpulibs.Col.from_list(low), "upper": cpulibs.Col.from_list(up)}


@pytest.mark.parametrize("rowwise", [False, True], ids=["tile", "rows"])
@pytest.mark.parametrize("op", cm.OPS)
def test_malformed_rows_that_keep_their_size(keeping, monkeypatch, op, rowwise):
    """arbitrary bytes the oracle reports as size-keeping, so that the tile kernel's answer is the one returned: lead
    bytes that swallow ASCII letters, stray continuation bytes, surrogates, and characters cut off by the end of their row
    in front of an ASCII row (a patch running past its row would land there).  With CS_CASE_ROWWISE the row kernels answer
    the same column: both routes are held to the oracle."""
    if rowwise:
        monkeypatch.setenv("CS_CASE_ROWWISE", "1")
    _, col, want = keeping
    check(op, col, want[op], "rows" if rowwise else "tile")


# ---- 4: tile shapes -----------------------------------------------------------------------------------------------------------
ALPHABET = [ch.encode() for ch in "abcXYZ 09.qQéÉḀḁ"]
SHAPES = {"R64": (0, 90), "R32": (100, 180), "R16": (200, 370)}  # row sizes at which 64, 32, 16 rows fit the staging buffer


def _text_rows(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for size in rng.integers(lo, hi + 1, n).tolist():
        r = b""
        for k in rng.integers(0, len(ALPHABET), size).tolist():
            if len(r) + len(ALPHABET[k]) > size:
                break
            r += ALPHABET[k]
        rows.append(r + b"q" * max(0, lo - len(r)))
    return rows


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 256, 257, 319])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tile_shapes(orc, shape, nrows):
    """rows of ASCII, é and Ḁ (keepers) sized for 64-, 32- and 16-row tiles, at row counts that end in a partial tile and
    at tile counts that are no multiple of the four waves of a workgroup"""
    lo, hi = SHAPES[shape]
    rows = _text_rows(nrows, lo, hi, 100 + nrows)
    assert not set(ord(c) for c in "éÉḀḁ") & (set(cm.changers("lower")) | set(cm.changers("upper")))
    col = cpulibs.Col.from_list(rows)
    text = [r.decode() for r in rows]
    for op in cm.OPS:
        check(op, col, getattr(orc, op)(col), "tile", model=cpulibs.Col.from_list(cm.case_column(op, text)))


# ---- 5: tiles beyond the staging buffer --------------------------------------------------------------------------------------
LONG = 7000


def _long_malformed(keeping, orc):
    """Kept rows of item 3 joined to one row of 7,000 bytes that still keeps its size, by the ORACLE.  Joining is not free:
    behind a stray continuation byte the reference's walk stands still, so only rows without continuation bytes can follow
    one.  Hence rows the walk passes cleanly first (the row still keeps its size with a well-formed character appended),
    then malformed rows while the row keeps its size with them, then ASCII rows up to the size."""
    crafted = set(cm.truncated_tails())
    kept = [r for r in keeping[0] if r not in crafted]

    def keeps(row):
        one = cpulibs.Col.from_list([row])
        return len(orc.lower(one).chars) == len(row) and len(orc.upper(one).chars) == len(row)

    row, malformed = b"", 0
    for r in kept:
        if len(row) >= LONG - 400:
            break
        if keeps(row + r + "é".encode()):
            row += r
    for r in kept:
        if len(row) >= LONG:
            break
        if not cm.is_utf8(r) and keeps(row + r):
            row += r
            malformed += 1
    for r in kept:
        if len(row) >= LONG:
            break
        if r.isascii() and keeps(row + r):
            row += r
    assert len(row) >= LONG and keeps(row) and malformed >= 1 and not cm.is_utf8(row), (len(row), malformed)
    return row


def _model(op, rows):
    """the model's answer for rows of well-formed bytes (a repeated row is mapped once)"""
    memo = {r: cm.case_row(op, r.decode()).encode() for r in set(rows)}
    return cpulibs.Col.from_list([memo[r] for r in rows])


@pytest.mark.parametrize("kind", ["ascii", "accents", "malformed", "first", "last", "changer"])
def test_oversize_tile(orc, keeping, kind):
    """one 7,000-byte row among 2,000 short ones: its tile is mapped straight from memory (map_span_from_memory), the rows
    of that tile redone a thread each when it holds non-ASCII bytes; a changer in the long row hands the column over"""
    short = _text_rows(2000, 0, 40, 9)
    accents = ("é1 " * 7 + "Ḁb" * 5).encode()  # 48 bytes
    for op in cm.OPS:
        if kind == "ascii":
            long_row = (b"xY z9 Q." * 1000)[:LONG]
        elif kind == "malformed":
            long_row = _long_malformed(keeping, orc)
        else:
            long_row = (accents * 300)[:LONG]
        if kind == "changer":
            ch = {"lower": "İ", "upper": "ß"}[op]
            assert ord(ch) in cm.changers(op)
            long_row = long_row[:48 * 73] + ch.encode() + long_row[48 * 73:]
        rows = list(short)
        rows[{"first": 0, "last": len(rows) - 1}.get(kind, 1000)] = long_row
        col = cpulibs.Col.from_list(rows)
        check(op, col, getattr(orc, op)(col), "rows" if kind == "changer" else "tile", model=None if kind == "malformed" else _model(op, rows))


def test_no_tile_fits(orc):
    """600 rows of 9 and 12 KB, no tile of any size fits the staging buffer.  The column takes the TILE route: the plan
    allows outlier tiles without counting them, and every tile is mapped from memory."""
    rows = [(b"xY z9 " * 2000) if i % 3 else ("Ünï " * 1500).encode() for i in range(600)]
    col = cpulibs.Col.from_list(rows)
    for op in cm.OPS:
        took = check(op, col, getattr(orc, op)(col), None, model=_model(op, rows))
        assert took == "tile"


# ---- 6: chars that start inside a 16-byte piece -------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 7, 13])
@pytest.mark.parametrize("op", cm.OPS)
def test_shifted_chars_buffer(orc, op, shift):
    """a borrowed column whose chars start `shift` bytes past a 16-byte boundary, 0xFF bytes in front and behind: the first
    tile's `lead` is not zero, and the bits the bitmap holds for the bytes around the column are no row's"""
    rows = _well_formed(op, "packed")[0][:1500] + _well_formed(op, "embedded")[0][:3000]
    enc = [r.encode() for r in rows]
    b = bu.Borrowed(enc, shift, 8, bu.poison_for("ff", "lower"))
    col = cpulibs.Col.from_list(enc)
    check(op, col, getattr(orc, op)(col), "tile", g=b.col, model=cpulibs.Col.from_list(cm.case_column(op, rows)))
    assert b.caller_memory_intact()
