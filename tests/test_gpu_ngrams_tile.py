"""create_ngrams on the MI355X against the oracle and the Python model of tests/tokens_model.py, with the route proven
(cs_debug_last_route): k_ngram_tile (cs_ngram.hip) with separators of 0 to 8 bytes and n = 2 to 8 (9 of either: row-wise),
rows == n (the join) and n + 1, tokens of 15, 16 and 17 bytes around or_bytes' hand-over to lds_copy, tokens at every source
and destination alignment, every M with a last tile of 1, 63, 64 and 65 n-grams, columns that force M = 2 and M = 1 and one
that fits none, a null or an empty row at the first, a middle and the last position, token columns made by tokenize (born
without dropped rows) and plain ones (asked once), twice over, and borrowed columns whose chars start inside a 16-byte piece.
tests/test_tokens_model_cpu.py proves the expected values.

Every comparison is byte-exact on chars, int64 offsets and validity, against both; the route is the model's M for the column;
the input's digest and the fallback count do not move; every case runs once more with CS_NGRAM_ROWWISE, where the route is
"rows" and the output the same."""
import numpy as np
import pytest

import borrowedutil as bu
import cpulibs
import gpuutil
import tokens_model as tm

pytestmark = pytest.mark.gpu

NG_CASES = tm.ng_cases()


@pytest.fixture(scope="module")
def orc():
    return cpulibs.Oracle()


def check(orc, monkeypatch, rows, n, sep, m_first, route, g=None):
    from custrings_amd import nvtext

    L = gpuutil.lib()
    col = cpulibs.Col.from_list(rows)
    g = g if g is not None else gpuutil.from_col(col)
    before, f0 = g.digest(), L.lib.cs_fallback_count()
    refs = {"oracle": orc.ngrams(col, n, sep), "model": cpulibs.Col.from_list(tm.ngrams(rows, n, sep))}
    if m_first != 8:
        monkeypatch.setenv("CS_NGRAM_M", str(m_first))
    for rowwise in (False, True):
        if rowwise:
            monkeypatch.setenv("CS_NGRAM_ROWWISE", "1")
        for again in (0, 1):  # (the second call finds what the first remembered on the column)
            out = nvtext.ngrams(g, n, sep.decode())
            took = L.lib.cs_debug_last_route().decode()
            assert took == ("rows" if rowwise else route), (n, sep, again, took)
            got = gpuutil.to_col(out)
            for name, want in refs.items():
                gpuutil.same_tokens(got, want, (n, sep, took, again, name))
    monkeypatch.delenv("CS_NGRAM_ROWWISE")
    monkeypatch.delenv("CS_NGRAM_M", raising=False)
    assert g.digest() == before and L.lib.cs_fallback_count() == f0


@pytest.mark.parametrize("case", NG_CASES, ids=[c.name for c in NG_CASES])
def test_ngrams(orc, monkeypatch, case):
    rows = case.build()
    check(orc, monkeypatch, rows, case.n, case.sep, case.m_first, tm.ng_route(case, rows))


@pytest.mark.parametrize("n,sep", [(2, b"_"), (3, b""), (8, b"12345678")])
def test_ngrams_of_tokenize_output(orc, monkeypatch, n, sep):
    """the token column as tokenize makes it -- tile and row-wise -- goes straight into ngrams"""
    from custrings_amd import nvtext

    column = tm.col_tok_shape("R32")
    tokens, _ = tm.tokenize_column(column.rows, None)
    route = tm.ngram_route(tokens, n, sep)
    assert route.startswith("tile-m")
    for var in (None, "CS_TOKENIZE_ROWWISE"):
        if var:
            monkeypatch.setenv(var, "1")
        g = nvtext.tokenize(gpuutil.from_col(column.col()))
        monkeypatch.delenv("CS_TOKENIZE_ROWWISE", raising=False)
        check(orc, monkeypatch, tokens, n, sep, 8, route, g=g)


@pytest.mark.parametrize("shift", [1, 7, 13])
def test_shifted_chars_buffer(orc, monkeypatch, shift):
    """a borrowed token column whose chars start `shift` bytes past a 16-byte boundary: every tile's `lead` moves, and with
    it every token's source alignment"""
    rows = tm.toks_lengths(64 * 4 + 9)
    b = bu.Borrowed(rows, shift, 8, bu.poison_for("ff", "text"))
    for n, sep in ((2, b"_"), (3, b"+-+")):
        check(orc, monkeypatch, rows, n, sep, 8, tm.ngram_route(rows, n, sep), g=b.col)
    assert b.caller_memory_intact()
