"""split_re / rsplit_re without a GPU: the model of tests/splitre_model.py pinned by two identities on the CPU oracle --
a one-byte literal splits as split / rsplit do, and split_re(pat, n) is split(replace_re(pat, SEP, n), SEP, n) -- and
custrings_amd/csrc/splitre_ops.h (the text the kernel compiles), built with g++, against the model."""
import pytest

import splitre_model as m

ROWS = ["a, b;c", None, "", ",lead", "trail;", "a,,b", ",", "é , é;x  ;", "nul\x00a , b,c", "one two  three 42 x7y,8"]
PATTERNS = [r"\s*[,;]\s*", ",", r"\s+", "[,;]+", r"\d+"]
LIMITS = [-1, 1, 2, 3]


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("pat", PATTERNS)
def test_model_is_split_of_replace_re(pat, limit):
    orc = m.oracle()
    want = orc.split(orc.replace_re(ROWS, pat, m.SEP, limit), m.SEP, limit)
    assert m.columns(ROWS, pat, limit) == want


def test_model_literal_is_split():
    orc = m.oracle()
    assert m.columns(ROWS, ",") == orc.split(ROWS, ",")
    assert m.columns(ROWS, ",", 2, reverse=True) == orc.rsplit(ROWS, ",", 2)


@pytest.mark.parametrize("limit", LIMITS)
def test_model_literal_is_split_with_a_limit(limit):
    orc = m.oracle()
    assert m.columns(ROWS, ",", limit) == orc.split(ROWS, ",", limit)
    assert m.columns(ROWS, ",", limit, reverse=True) == orc.rsplit(ROWS, ",", limit)


def test_model_edges():
    assert m.columns([], ",") == [[]]
    assert m.columns([None, None], ",") == [[None, None]]
    assert m.columns(["", None], ",") == [["", None]]
    assert m.records(["a,b,c", None, ",", "x"], ",", 1) == [["a", "b,c"], None, ["", ""], ["x"]]
    assert m.records(["a,b,c", None, ",", "x"], ",", 1, reverse=True) == [["a,b", "c"], None, ["", ""], ["x"]]
    # the matches are found left to right whichever end cuts: "aaa" holds one match of "aa", at the front
    assert m.records(["aaa"], "aa", 1, reverse=True) == [["", "a"]]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return m.Harness(str(tmp_path_factory.mktemp("splitre")))


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("limit", [-1, 0, 1, 2, 3, 4, 99])
def test_ops_header_against_model(harness, limit, reverse):
    rows = [r for r in ROWS if r is not None] + ["a,b,c,d", ",,,", "x"]
    for pat in PATTERNS:
        spans = m.match_spans(rows, pat)
        want = m.records(rows, pat, limit, reverse)
        ncols = max(len(r) for r in want) + 1  # (one column past the widest row: null for every row)
        assert harness.records(rows, spans, limit, reverse, ncols) == want, (pat, limit, reverse)
