"""tokenize on the MI355X against the oracle and the Python model of tests/tokens_model.py, with the route proven
(cs_debug_last_route): k_tok_tile<PASS, SEGS> (cs_tokenize.hip) in whitespace mode and with sets of one to four ASCII
delimiters, the three tile sizes at a partial last tile, an oversize tile walked in segments with a row, a token and a
character at the segment boundaries, multi-byte characters across 16-byte pieces, 1024-byte chunk rows, rows and tiles,
tokens that open a row behind a kept byte, tiles and a whole column without a token, one malformation at each edge of the
kernel's UTF-8 check, arbitrary bytes, and borrowed columns whose chars start inside a 16-byte piece.
tests/test_tokens_model_cpu.py proves the expected values.

Every comparison is byte-exact on chars, int64 offsets and validity; the route is the one the case's table fixes; the input's
digest and the fallback count do not move; every case runs once more with CS_TOKENIZE_ROWWISE, where the route is "rows" and
the output the same.  The whole column is held to the model's statement of what the project does where the reference reads
behind a row (tokens_model.walk(strict=False)); the column without those rows is held to the oracle and the strict model."""
import numpy as np
import pytest

import borrowedutil as bu
import cpulibs
import gpuutil
import rows_model as rm
import tokens_model as tm

pytestmark = pytest.mark.gpu

TOK_CASES = tm.tok_cases()


@pytest.fixture(scope="module")
def orc():
    return cpulibs.Oracle()


def tokens_col(tokens):
    return cpulibs.Col.from_list(tokens)


def check(orc, monkeypatch, column, delims, route, outliers=True, g=None, base=0):
    from custrings_amd import nvtext

    L = gpuutil.lib()
    if not outliers:
        monkeypatch.setenv("CS_NO_OUTLIER_TILES", "1")
    g = g if g is not None else gpuutil.from_col(column.col())
    before, f0 = g.digest(), L.lib.cs_fallback_count()
    for delim in delims:
        want_route = tm.tok_route(column.rows, delim, base, outliers)
        assert want_route == ("rows" if delim in tm.ROWS_SETS else route), (delim, want_route)
        lenient, _ = tm.tokenize_column(column.rows, delim, strict=False)
        strict, undefined = tm.tokenize_column(column.rows, delim)
        gone = set(undefined)
        defined = rm.Column([r for i, r in enumerate(column.rows) if i not in gone]).col()
        sub = gpuutil.from_col(defined) if undefined else None
        oracle = orc.tokenize(defined, delim)
        gpuutil.same_tokens(oracle, tokens_col(strict), (delim, "oracle against model"))
        for rowwise in (False, True):
            if rowwise:
                monkeypatch.setenv("CS_TOKENIZE_ROWWISE", "1")
            out = nvtext.tokenize(g, delim)
            took = L.lib.cs_debug_last_route().decode()
            assert took == ("rows" if rowwise else want_route), (delim, took)
            got = gpuutil.to_col(out)  # (_export64: int64 offsets)
            gpuutil.same_tokens(got, tokens_col(lenient), (delim, took, "model"))
            if sub is None:
                gpuutil.same_tokens(got, oracle, (delim, took, "oracle"))
            else:
                gpuutil.same_tokens(gpuutil.to_col(nvtext.tokenize(sub, delim)), oracle, (delim, took, "oracle, defined rows"))
            if rowwise:
                monkeypatch.delenv("CS_TOKENIZE_ROWWISE")
    monkeypatch.delenv("CS_NO_OUTLIER_TILES", raising=False)
    assert g.digest() == before and L.lib.cs_fallback_count() == f0


@pytest.mark.parametrize("case", TOK_CASES, ids=[c.name for c in TOK_CASES])
def test_tokenize(orc, monkeypatch, case):
    """the table of tests/tokens_model.py::tok_cases; every column also with five delimiters and -- but for the columns with
    a row that ends in a cut character, which the set "é " leaves undefined -- with a non-ASCII set, both row-wise"""
    extra = ["abcde"] if case.name.startswith("malformed-") else tm.ROWS_SETS
    check(orc, monkeypatch, case.build(), case.delims + extra, case.route, case.outliers)


@pytest.mark.parametrize("shift", [1, 7, 13])
@pytest.mark.parametrize("shape", ["R64", "R32", "R16", "segs"])
def test_shifted_chars_buffer(orc, monkeypatch, shape, shift):
    """a borrowed column whose chars start `shift` bytes past a 16-byte boundary, 0xFF bytes around: every tile's `lead`
    moves, and with it the piece, chunk row and segment a byte falls into"""
    column = tm.col_tok_segs() if shape == "segs" else rm.Column(tm.col_tok_shape(shape).rows)
    route = tm.tok_plan(column.offsets(), base=shift).route
    assert route == ("tile-segs" if shape == "segs" else "tile")
    b = bu.Borrowed(column.rows, shift, 8, bu.poison_for("ff", "text"))
    check(orc, monkeypatch, column, [None, " ", "_- "], route, g=b.col, base=shift)
    assert b.caller_memory_intact()
