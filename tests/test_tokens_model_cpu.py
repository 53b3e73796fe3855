"""The Python model of tokenize / create_ngrams (tests/tokens_model.py) against the oracle, and the host emulation of the
row-wise kernels (tests/rowemu, compiled from row_ops.h) against the model, on every column and every parameter set that
tests/test_gpu_tokenize_tile.py and tests/test_gpu_ngrams_tile.py run; every generator's plan -- tile size, segments, route, M
-- restated from the offsets.  Proves the expected values with no GPU.

The oracle is only ever asked about rows the model calls defined: where the reference reads behind a row, the oracle's
restatement of it may read anything.  Those rows are counted, and may be no more than a third of a column's malformed rows."""
import numpy as np
import pytest

import cpulibs
import rows_model as rm
import tokens_model as tm


@pytest.fixture(scope="module")
def orc():
    return cpulibs.Oracle()


@pytest.fixture(scope="module")
def emu():
    return cpulibs.RowEmu()


TOK_CASES = tm.tok_cases()
NG_CASES = tm.ng_cases()


def first_difference(a, b):
    return next(((i, a[i], b[i]) for i in range(min(len(a), len(b))) if a[i] != b[i]), (min(len(a), len(b)), len(a), len(b)))


def check_tokenize(orc, emu, c, delim):
    want, undefined = tm.tokenize_column(c.rows, delim)
    malformed = tm.malformed_rows(c.rows)
    assert 3 * len(undefined) <= len(malformed), (delim, len(undefined), len(malformed))
    gone = set(undefined)
    defined = rm.Column([r for i, r in enumerate(c.rows) if i not in gone])
    got = orc.tokenize(defined.col(), delim).to_bytes_list()
    assert got == want, (delim,) + first_difference(got, want)
    lenient, none = tm.tokenize_column(c.rows, delim, strict=False)
    assert none == []
    got = emu.tokenize(c.col(), delim).to_bytes_list()
    assert got == lenient, (delim,) + first_difference(got, lenient)
    return len(undefined), len(malformed)


@pytest.mark.parametrize("case", TOK_CASES, ids=[c.name for c in TOK_CASES])
def test_tokenize_model_equals_oracle_and_rowemu(orc, emu, case):
    c = case.build()  # (asserts the column's plan)
    assert 0 < len(c.rows) <= 5000
    # (a row that ends in C3 is undefined with the set "é ": the byte behind it decides)
    for delim in case.delims + (["abcde"] if case.name.startswith("malformed-") else tm.ROWS_SETS):
        want = "rows" if delim in tm.ROWS_SETS else case.route
        assert tm.tok_route([r for r in c.rows], delim, outliers=case.outliers) == want, (delim, want)
        check_tokenize(orc, emu, c, delim)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_arbitrary_bytes(orc, emu, seed):
    """rows of 0 to 11 bytes from the pool "ab c\\t" + 00 C3 A9 E2 82 80 1F F0, whitespace and three sets; rows with a
    non-ASCII set as well, where a stray continuation byte that a member holds is a delimiter"""
    c = tm.col_tok_malformed(seed=seed)
    for delim in (None, " ", " .", "_-", "é "):
        u, m = check_tokenize(orc, emu, c, delim)
        assert m > 3000 and u > 0  # (the pool does reach what the reference leaves undefined)


def test_rows_the_issue_quotes():
    f = bytes.fromhex
    assert tm.tokens_of(f("821f")) == [f("821f")]
    assert tm.tokens_of(f("ff00a9a9")) == [f("ff00a9a9")]
    assert tm.tokens_of(f("62f01fe2ff80")) == [f("62f01fe2ff80")]
    assert tm.tokens_of(f("e2208080f88009")) == [f("e2208080f88009")]  # (E2 takes 20 80 with it; the iterator stays on the second 80)
    with pytest.raises(tm.Undefined):
        tm.tokens_of(f("c3e2206180"))  # the second token would begin at byte 5 of 5
    assert tm.tokens_of(f("a9")) == []                        # no character at all
    assert tm.tokens_of(f("61802062")) == [f("61802062")]      # the iterator never leaves the stray 80
    assert tm.tokens_of(f("61a962"), "é") == [b"a"] and tm.tokens_of(f("61a962"), " ") == [f("61a962")]  # A9 is found in the delimiter string C3 A9
    assert tm.tokens_of(b"a\0b", None) == [b"a", b"b"] and tm.tokens_of(b"a\0b", " ") == [b"a\0b"]
    assert tm.well_formed(f("f8808080")) and rm.as_text(f("f8808080")) is None and not tm.well_formed(f("c3"))


def test_plans_restate_the_thresholds():
    offs = lambda sizes: np.concatenate([[0], np.cumsum(sizes)])  # noqa: E731
    assert tm.tok_plan(offs([96] * 63 + [80])).R == 64 and tm.tok_plan(offs([96] * 63 + [81])).R == 32
    assert tm.tok_plan(offs([383] * 64)).R == 16 and tm.tok_plan(offs([383] * 63 + [384])).route == "tile-segs"
    assert tm.tok_plan(offs([6144, 1]), base=0).segs == [2] and tm.tok_plan(offs([6143]), base=1).route == "tile-segs"
    assert tm.tok_plan(offs([7000]), outliers=False).route == "rows" and tm.tok_plan(offs([])).route == "rows"
    assert tm.tok_route([b"a b"], "abcde") == "rows" and tm.tok_route([b"a b"], "abcd") == "tile"
    assert tm.tok_route([b"a b"], "é") == "rows" and tm.tok_route([b"a\xc3"], None) == "rows"
    assert tm.ngram_m(offs([3] * 600), 2, 0) == 8 and tm.ngram_m(offs([3] * 600), 2, 0, m_first=2) == 2
    assert tm.ngram_m(offs([5] * 600), 2, 1) == 4   # eight a lane fit, but not four workgroups: four a lane
    assert tm.ngram_m(offs([3] * 600), 9, 1) == 0 and tm.ngram_m(offs([3] * 600), 2, 9) == 0 and tm.ngram_m(offs([3] * 2), 2, 1) == 0


@pytest.mark.parametrize("case", NG_CASES, ids=[c.name for c in NG_CASES])
def test_ngrams_model_equals_oracle(orc, case):
    rows = case.build()
    assert 0 < len(rows) <= 5000
    tm.ng_route(case, rows)  # (asserts the route the table fixes against the restated M)
    got = orc.ngrams(cpulibs.Col.from_list(rows), case.n, case.sep).to_bytes_list()
    want = tm.ngrams(rows, case.n, case.sep)
    assert got == want, first_difference(got, want)


def test_ngram_generators_reach_their_edges():
    lens = {len(t) for t in tm.toks_lengths(64 * 2 + 5)}
    assert {15, 16, 17, 33, 1} <= lens
    toks = tm.toks_lengths(64 * 2 + 5)
    offs = rm.Column(toks).offsets()
    assert {int(o) & 3 for o in offs[:-1]} == {0, 1, 2, 3}  # every source alignment
    # or_bytes, by construction and not by luck of the draw: every (source, destination) alignment; at every destination
    # alignment sd a token with len + sd <= 8 and one of 9 to 16 bytes (the __any branch: the words behind the second), and
    # a wave -- 64 consecutive n-grams -- that holds both; tokens of 15, 16 and 17 bytes at every destination alignment
    for n, sepn in ((3, 1), (3, 0), (2, 1)):
        m = tm.ngram_m(offs, n, sepn)
        calls = tm.or_bytes_calls(toks, n, sepn, m)
        assert {(si, di) for si, di, _ in calls} == {(a, b) for a in range(4) for b in range(4)}, (n, sepn)
        for sd in range(4):
            assert any(di == sd and ln + sd <= 8 for _, di, ln in calls) and any(di == sd and 9 <= ln <= 16 for _, di, ln in calls)
            assert {15, 16, 17} <= {ln for _, di, ln in calls if di == sd}, (n, sepn, sd)
        per_wave = [calls[i:i + 64 * n] for i in range(0, len(calls), 64 * n)]
        assert any(min(ln + di for _, di, ln in w) <= 8 < max(ln + di for _, di, ln in w) for w in per_wave)
    for size in (15, 16, 17):  # the columns of one size: 16 goes through or_bytes alone, 17 hands one byte to lds_copy
        calls = tm.or_bytes_calls(tm.toks_sized(200, size), 2, 1, tm.ngram_m(rm.Column(tm.toks_sized(200, size)).offsets(), 2, 1))
        assert {ln for _, _, ln in calls} == {size} and {di for _, di, _ in calls} == {0, 1, 2, 3}
    routes = {tm.ng_route(c, c.build()) for c in NG_CASES}
    assert routes == {"rows", "tile-m8", "tile-m4", "tile-m2", "tile-m1"}
    assert tm.ngrams([b"a", None, b"", b"b"], 2, b"_") == [b"a___b"] and tm.ngrams([b"a", None, b"b", b"c"], 2, b"-") == [b"a-b", b"b-c"]
    assert tm.ngrams([b"a", None, b"b"], 1, b"_") == [b"a", None, b"b"] and tm.ngrams([], 2, b"_") == []
