"""contains_strings / strings_counts / edit_distance / porter_stemmer_measure / scatter_count without a GPU: the Python model
(tests/text_model.py) and text_ops.h (the text the kernels compile) built with g++ against the reference's known answers and
the quirks of DESIGN.md section 4f; the bit-vector form of edit_distance against the dynamic program on about 1M generated
pairs; the dynamic program against the model; the relink of the six NVText members; the pyni names; the Python API."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cpulibs
import text_model as m

ROOT = cpulibs.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_text.json")


def cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_golden_covers_every_member_and_source():
    assert {c["op"] for c in cases()} == set(m.MEMBERS)
    assert {c["src"].split(":")[0] for c in cases()} == {"cpp/tests/test_text.cu", "python/tests/test_text.py"}


@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s" % (c["op"], c["src"].split("/")[-1]))
def test_model_reproduces_known_answers(case):
    assert m.apply_case(case) == case["expected"], case["src"]


@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


def test_harness_reproduces_known_answers(harness):
    for case in cases():
        assert harness.apply_case(case) == case["expected"], case["src"]


# ---- the quirks, each with an answer derived by hand -------------------------------------------------------------------------
def _both(harness):
    return [m, harness]


def test_counts_restart_behind_the_match(harness):
    for impl in _both(harness):
        # "aa" at 0, the next search starts 2 characters on: at 2; "aaa": found at 0, restart at 3: one byte left
        assert impl.strings_counts(["aaaa", "aaaaa", "aaa"], ["aa", "aaa"]) == [[2, 1], [2, 1], [1, 1]]


def test_a_target_matches_across_a_character_boundary(harness):
    # "é" = C3 A9, "©" = C2 A9, "Ã" = C3 83.  The target A9 C3 (no valid string: the tail of "é" and the head of the next "é")
    # occurs in the BYTES of "éé" at byte 1; one character ("é") starts in front of it: position 1.
    rows = ["éé".encode(), "©Ã".encode(), "e".encode()]
    tgt = [b"\xa9\xc3"]
    assert harness.contains_strings(rows, tgt) == [[True], [True], [False]]
    # counts: the target holds one character start (C3), so the next search starts at character 1 + 1 = 2 = the row's end
    assert harness.strings_counts(rows, tgt) == [[1], [1], [0]]
    # "éaéaé" = C3 A9 61 C3 A9 61 C3 A9 (5 characters); the target A9 61 (one character start) matches at bytes 1 and 4.
    # Byte 1: 1 character starts in front -> position 1, restart at character 2 = byte 3.  Byte 4: 3 start in front (C3, 61, C3)
    # -> position 3, restart at character 4 = byte 6: no match there.
    assert harness.strings_counts(["éaéaé".encode()], [b"\xa9a"]) == [[2]]
    # "aéaé" = 61 C3 A9 61 C3 A9 (4 characters); the target 61 C3 holds two character starts.  Byte 0: position 0, restart at
    # character 2 = byte 3, where it matches again: position 2, restart at character 4 = the row's end.
    assert harness.strings_counts(["aéaé".encode()], [b"a\xc3"]) == [[2]]
    # multi-byte characters in front of a match shift the restart: row "ééaa", target "a": 2
    for impl in _both(harness):
        assert impl.strings_counts(["ééaa", "日本日本"], ["a", "本", "日本"]) == [[2, 0, 0], [0, 2, 2]]
        assert impl.contains_strings(["ééaa"], ["éa", "ae"]) == [[True, False]]


def test_empty_and_null_targets_and_rows(harness):
    for impl in _both(harness):
        assert impl.contains_strings(["abc", "", None], ["", None, "abc", "abcd"]) == [[False, False, True, False], [False] * 4, [False] * 4]
        assert impl.strings_counts(["abc", "", None], ["", None, "abc", "abcd"]) == [[0, 0, 1, 0], [0] * 4, [0] * 4]


def test_edit_distance_of_null_and_empty_sides(harness):
    for impl in _both(harness):
        assert impl.edit_distance([None, "", "añb", "x"], "日本語") == [3, 3, 3, 3]
        assert impl.edit_distance([None, "", "añb"], "") == [0, 0, 3]
        assert impl.edit_distance([None, "", "añb", None, "", "añb", "añb"], ["日本", "日本", None, None, None, "", "añb"]) == [2, 2, 3, 0, 0, 3, 0]
    assert harness.edit_distance([None, "", "añb", "x"], "日本語", form="bits") == [3, 3, 3, 3]


def test_edit_distance_counts_characters_not_bytes(harness):
    for impl in _both(harness):
        assert impl.edit_distance(["é", "e", "éé", "日本"], "e") == [1, 0, 2, 2]
        assert impl.edit_distance(["kitten", "sitting", "Saturday"], ["sitting", "kitten", "Sunday"]) == [3, 3, 3]
    assert harness.edit_distance(["é", "e", "éé", "日本"], "e", form="bits") == [1, 0, 2, 2]
    assert harness.edit_distance(["e", "é", "ée", "日é本"], "é", form="bits") == [1, 0, 1, 2]


def test_measure_of_y(harness):
    for impl in _both(harness):
        # "y": a consonant at index 0.  "yy": the second y follows a consonant, so it counts as a vowel: a run, never closed.
        # "ay": y behind a vowel is a consonant and closes the run.  "yay": y a y -> consonant, vowel, consonant: 1.
        assert impl.porter_stemmer_measure(["y", "yy", "ay", "", None, "yay", "syzygy", "tree", "trees"]) == [0, 0, 1, 0, 0, 1, 2, 0, 1]
        assert impl.porter_stemmer_measure(["añb", "ñaña", "bèbéb"], vowels="aèé", y_char="ñ") == [1, 1, 2]
        # more than eight non-ASCII vowels (the ninth and tenth take the list in memory)
        assert impl.porter_stemmer_measure(["bàbùbÿb", "ÿb", "bÿ"], vowels="àáâãäåæèéùÿ", y_char="y") == [3, 1, 0]


def test_scatter_count_of_zero_counts_and_null_rows(harness):
    for impl in _both(harness):
        assert impl.scatter_count(["a", None, "c", ""], [0, 2, 0, 3]) == [None, None, "", "", ""]
        assert impl.scatter_count(["a", None], [0, 0]) == []
        assert impl.scatter_count(["a", "b", "c"], [None, 1, None]) == ["b"]


# ---- the bit-vector form against the dynamic program ---------------------------------------------------------------------------
PAIRS = 1_000_000
TARGET_CHARS = [1, 2, 31, 32, 33, 63, 64]
ALPHABETS = [["a", "b", "c", "d"], ["a", "b", "é", "日"]]


@pytest.mark.parametrize("tchars", TARGET_CHARS)
def test_bit_vector_form_matches_dynamic_program(harness, tchars):
    per_target = 10
    rows_each = PAIRS // (len(TARGET_CHARS) * per_target) + 1
    rng = np.random.default_rng(100 + tchars)
    for k in range(per_target):
        alphabet = ALPHABETS[k % 2]
        rows = m.letter_rows(rows_each, seed=1000 * tchars + k, alphabet=alphabet, max_len=100)
        target = "".join(alphabet[i] for i in rng.integers(0, 4, size=tchars).tolist())
        tg = m.to_arrow([target])
        dp = harness.run_arrow("edit_scalar", rows, tg, "dp")
        bits = harness.run_arrow("edit_scalar", rows, tg, "bits")
        bad = np.flatnonzero(dp != bits)
        assert bad.size == 0, (target, bad[:5], dp[bad[:5]], bits[bad[:5]])
        assert len(set(dp.tolist())) >= 3, target  # (the distances vary)
        assert int(dp.max()) <= max(100, tchars) and int(dp.min()) >= 0


def test_dynamic_program_matches_model(harness):
    n = 20_000
    rng = np.random.default_rng(5)
    letters = ["a", "b", "é", "日", "c"]

    def word(k):
        return "".join(letters[i] for i in rng.integers(0, len(letters), size=k).tolist())

    la, lb = rng.integers(0, 13, size=n).tolist(), rng.integers(0, 13, size=n).tolist()
    a = [None if x == 12 else word(x) for x in la]
    b_ = [None if x == 12 else word(x) for x in lb]
    want = m.edit_distance(a, b_)
    assert harness.edit_distance(a, b_) == want
    assert harness.edit_distance(a, b_, form="bits") == want
    assert len(set(want)) > 8


def test_harness_matches_model_on_generated_rows(harness):
    rows = m.gen_rows(30_000, seed=3)
    targets = ["the", "a", "aa", "é", "日本", "y ", "", None, "queue"]
    assert harness.contains_strings(rows, targets) == m.contains_strings(rows, targets)
    counts = m.strings_counts(rows, targets)
    assert harness.strings_counts(rows, targets) == counts
    assert max(max(r) for r in counts) >= 3
    for vowels, y in (("aeiou", "y"), ("aeiouéü", "ÿ")):
        want = m.porter_stemmer_measure(rows, vowels, y)
        assert harness.porter_stemmer_measure(rows, vowels, y) == want
        assert max(want) >= 4
    cnt = np.random.default_rng(4).integers(0, 4, size=len(rows)).tolist()
    assert harness.scatter_count(rows, cnt) == m.scatter_count(rows, cnt)


# ---- relink: a caller of the six members, compiled against the reference's headers ---------------------------------------------
CALLER = r"""
#include "NVStrings.h"
#include "NVText.h"
void calls(NVStrings& a, NVStrings& b, bool* f, unsigned int* u) {
  NVText::contains_strings(a, b, f); NVText::strings_counts(a, b, u);
  NVText::edit_distance(NVText::levenshtein, a, "x", u); NVText::edit_distance(NVText::levenshtein, a, b, u);
  NVText::porter_stemmer_measure(a, nullptr, nullptr, u); NVText::scatter_count(a, u);
}
"""
REF_INCLUDE = "/root/reference/cpp/include"
SYMBOLS = os.path.join(ROOT, "tests", "golden", "relink_text_symbols.json")


def caller_symbols(include_dir):
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "caller.cpp"), os.path.join(d, "caller.o")
        with open(src, "w") as f:
            f.write(CALLER)
        subprocess.run(["g++", "-std=c++14", "-c", "-I", include_dir, src, "-o", obj], check=True)
        out = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
        return sorted({ln.split()[-1] for ln in out.splitlines() if "NVText" in ln})


def wanted_symbols():
    with open(SYMBOLS) as f:
        return json.load(f)["symbols"]


def test_recorded_symbols_match_reference_headers():
    assert len(wanted_symbols()) == 6
    if not os.path.isdir(REF_INCLUDE):
        pytest.skip("the reference headers are not on this machine")
    assert caller_symbols(REF_INCLUDE) == wanted_symbols()


def test_our_headers_give_the_recorded_symbols():
    assert caller_symbols(os.path.join(ROOT, "include", "nvstrings")) == wanted_symbols()


def test_members_relink_against_libnvtext():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host"), "libs"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "custrings_amd", "libNVText.so")],
                         capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not (set(wanted_symbols()) - have), sorted(set(wanted_symbols()) - have)


# ---- the pyni glue names and the Python API ---------------------------------------------------------------------------------
PYNI = ["n_contains_strings", "n_strings_counts", "n_edit_distance", "n_scatter_count"]
API = ["contains_strings", "strings_counts", "edit_distance", "scatter_count", "porter_stemmer_measure"]


def test_pyni_names_are_what_the_reference_python_calls():
    with open(os.path.join(ROOT, "tests", "golden", "reference_python_calls.json")) as f:
        calls = json.dumps(json.load(f))
    for n in PYNI:
        assert '"%s"' % n in calls, n


def test_pyni_exports_the_new_names():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host")], check=True)
    code = "import pyniNVText as P; print(' '.join(n for n in %r if not hasattr(P, n)))" % PYNI
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "custrings_amd") + os.pathsep + ROOT)
    out = subprocess.run(["python3", "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == ""


def test_python_api_no_longer_refuses_them():
    import nvtext as top
    from custrings_amd import nvtext as N

    for n in API:
        assert callable(getattr(N, n)) and callable(getattr(top, n)) and n in N.__all__, n
    with pytest.raises(AttributeError):
        N.no_such_function


def test_c_abi_declares_and_exports_the_six_entries():
    from custrings_amd import _lib

    for n in ("cs_contains_strings", "cs_strings_counts", "cs_edit_distance", "cs_edit_distance_column", "cs_porter_stemmer_measure",
              "cs_scatter_count"):
        assert hasattr(_lib.lib, n) and n in _lib._PROTOS, n
