"""The character-type predicates and swapcase / capitalize / title without a GPU: the Python model (tests/chartype_model.py)
against the reference's known answers and the quirks of DESIGN.md section 4e; chartype_ops.h (the text the kernels compile)
built with g++ against the model on about 1M generated rows; the byte-parallel steps of the tile kernels against the sequential
routine; the relink of the twelve NVStrings members; the pyni names the reference's Python layer calls."""
import json
import os
import subprocess
import tempfile

import pytest

import chartype_model as m
import cpulibs

ROOT = cpulibs.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_chartype.json")


def cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def _model(case):
    if case["api"] == "python":
        return m.api_column(case["op"], case["input"])
    return [m.apply(case["op"], r) for r in case["input"]]


def test_golden_covers_every_member_and_source():
    assert {c["op"] for c in cases()} == set(m.MEMBERS)
    assert {c["src"].split(":")[0] for c in cases()} == {"cpp/tests/test_attrs.cu", "cpp/tests/test_case.cpp", "python/tests/test_case.py",
                                                          "python/tests/test_convert.py", "python/tests/test_allnulls.py"}


@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s" % (c["op"], c["src"].split("/")[-1]))
def test_model_reproduces_known_answers(case):
    assert _model(case) == case["expected"], case["src"]


def test_model_quirks():
    assert m.apply("islower", "123") and m.apply("isupper", "123")  # no alphabetic character: both
    for op in m.PREDS:
        assert m.apply(op, "") == (op == "is_empty") and m.apply(op, None) == (op == "is_empty"), op
        assert m.api_column(op, [None, ""]) == [None, op == "is_empty"]
        if op in m.MASKS:  # a four-byte character has flags 0: no bit, and not alphabetic (U+10400 is a cased letter elsewhere)
            assert m.apply(op, "\U0001F600") is False and m.apply(op, "a1\U00010400") is False, op
    assert m.apply("islower", "\U00010400") and m.apply("isupper", "\U00010400") and m.apply("islower", "a\U00010400")
    assert not m.apply("isupper", "a\U00010400") and m.apply("swapcase", "a\U00010400") == "A\U00010400"
    assert m.apply("is_empty", "\U0001F600") is False
    # U+2160 ROMAN NUMERAL ONE: upper, not alphabetic
    assert m.apply("islower", "aⅠ") and m.apply("isupper", "AⅠ") and not m.apply("isalpha", "Ⅰ")
    assert m.apply("title", "aⅠb") == "AⅠB" and m.apply("swapcase", "Ⅰ") == "ⅰ"
    # capitalize maps nothing above U+0FFF; title and swapcase do (Georgian, Latin Extended Additional)
    assert m.apply("capitalize", "ḁḀ") == "ḁḀ"
    assert m.apply("title", "ḁḀ") == "Ḁḁ" and m.apply("swapcase", "ḁḀ") == "Ḁḁ"
    assert m.apply("capitalize", "éÉ") == "Éé"
    assert m.apply("title", "o'neil mc-donald 1st") == "O'Neil Mc-Donald 1St"
    assert m.apply("title", "a1b") == "A1B" and m.apply("capitalize", "a1B") == "A1b"
    # width-changing characters: U+00DF -> 'S', U+0131 -> 'I', U+0130 -> 'i', U+017F -> 'S', U+212A -> 'k'
    assert m.apply("swapcase", "\u00df\u0131\u0130\u017f\u212a") == "SIiSk"
    assert m.apply("capitalize", "\u00dfx") == "Sx" and m.apply("capitalize", "x\u0130K") == "Xik"
    assert m.apply("capitalize", "x\u0130\u212a") == "Xi\u212a"  # (the Kelvin sign is above U+0FFF: capitalize leaves it)
    assert m.apply("title", "\u0131x \u017f\u0130 x\u212a") == "Ix Si Xk"
    assert len(m.width_changing()) == 98


# ---- the harness (chartype_ops.h) against the model ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


def test_harness_reproduces_known_answers(harness):
    for case in cases():
        got = harness.run(case["op"], m.encode(case["input"]))
        want = [m.apply(case["op"], r) for r in case["input"]]  # (the device's answer for a null row: False / True)
        if case["op"] in m.CASE_OPS:
            want = m.encode(case["expected"])
        else:
            assert [None if r is None else w for r, w in zip(case["input"], want)] == \
                   [None if r is None else e for r, e in zip(case["input"], case["expected"])]
        assert got == want, case["src"]


ROWS = 1_000_000


@pytest.fixture(scope="module")
def generated():
    return m.gen_rows(ROWS // len(m.MEMBERS) + 1, seed=3)


@pytest.mark.parametrize("op", m.MEMBERS)
def test_harness_matches_model_on_generated_rows(harness, generated, op):
    rows = generated
    got = harness.run(op, m.encode(rows))
    want = [m.apply(op, r) for r in rows]
    if op in m.CASE_OPS:
        want = m.encode(want)
    bad = [i for i in range(len(rows)) if got[i] != want[i]]
    assert not bad, [(rows[i], got[i], want[i]) for i in bad[:5]]
    if op in m.PREDS:
        assert 0 < sum(want) < len(rows)  # (both answers occur)


# ---- the tile kernels' byte-parallel steps against the sequential routine -----------------------------------------------
def _piece_rows():
    """every byte value in every position of a 16-byte piece, among letters, digits and blanks; rows of 16 bytes (pieces and rows
    coincide) and of 13 and 19 (every alignment of a row's start inside a piece, pieces across row boundaries)"""
    fillers = [b"aBcD eFgH1jKlMnOpQrS", b"ZYXWVUTSRQPONMLKJIHG", b"zz zz'zz-zz1zz zzzz ", b"                    "]
    rows = []
    for n in (16, 13, 19):
        for fill in fillers:
            for v in range(256):
                for k in range(n):
                    rows.append(fill[:k] + bytes([v]) + fill[k + 1:n])
    return rows


@pytest.mark.parametrize("op", m.CASE_OPS)
def test_byte_parallel_steps_match_the_sequential_routine(harness, op):
    rows = _piece_rows()
    seq = harness.run(op, rows)
    tile = harness.run(op, rows, mode="tile")
    changed = 0
    for r, a, b_ in zip(rows, seq, tile):
        if b_ == "CHANGED":
            assert len(a) != len(r), r
            changed += 1
        else:
            assert a == b_, (r, a, b_)
    assert changed < len(rows) // 4


@pytest.mark.parametrize("op", m.CASE_OPS)
def test_title_predecessor_rule_across_pieces_and_rows(harness, op):
    """letters and non-letters on both sides of every piece boundary and every row boundary, nulls and empty rows between"""
    rows = []
    for n in range(0, 40):
        for pat in (b"ab", b"a ", b" a", b"A1", b"Zz", b"'x"):
            rows.append((pat * 20)[:n])
        rows.append(None)
    rows += m.encode(m.gen_rows(40_000, seed=9, kind="ascii")) + m.encode(m.gen_rows(40_000, seed=10, kind="keep"))
    seq = harness.run(op, rows)
    tile = harness.run(op, rows, mode="tile")
    assert "CHANGED" not in tile  # (nothing here changes its width)
    bad = [i for i in range(len(rows)) if seq[i] != tile[i]]
    assert not bad, [(rows[i], seq[i], tile[i]) for i in bad[:5]]
    want = m.encode([None if r is None else m.apply(op, r.decode()) for r in rows])
    assert seq == want


# ---- relink: a caller of the twelve members, compiled against the reference's headers -------------------------------------
CALLER = r"""
#include "NVStrings.h"
void calls(NVStrings* s, bool* b) {
  s->isalnum(b); s->isalpha(b); s->isdigit(b); s->isspace(b); s->isdecimal(b); s->isnumeric(b); s->islower(b); s->isupper(b);
  s->is_empty(b); s->swapcase(); s->capitalize(); s->title();
}
"""
REF_INCLUDE = "/root/reference/cpp/include"
SYMBOLS = os.path.join(ROOT, "tests", "golden", "relink_chartype_symbols.json")


def caller_symbols(include_dir):
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "caller.cpp"), os.path.join(d, "caller.o")
        open(src, "w").write(CALLER)
        subprocess.run(["g++", "-std=c++14", "-c", "-I", include_dir, src, "-o", obj], check=True)
        out = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
        return sorted({ln.split()[-1] for ln in out.splitlines() if "NVStrings" in ln})


def wanted_symbols():
    with open(SYMBOLS) as f:
        return json.load(f)["symbols"]


def test_recorded_symbols_match_reference_headers():
    assert len(wanted_symbols()) == 12
    if not os.path.isdir(REF_INCLUDE):
        pytest.skip("the reference headers are not on this machine")
    assert caller_symbols(REF_INCLUDE) == wanted_symbols()


def test_our_headers_give_the_recorded_symbols():
    assert caller_symbols(os.path.join(ROOT, "include", "nvstrings")) == wanted_symbols()


def test_members_relink_against_libnvstrings():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host"), "libs"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "custrings_amd", "libNVStrings.so")],
                         capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not (set(wanted_symbols()) - have), sorted(set(wanted_symbols()) - have)


# ---- the pyni glue names and the Python API ---------------------------------------------------------------------------------
PYNI = ["n_" + n for n in m.MEMBERS]


def test_pyni_names_are_what_the_reference_python_calls():
    with open(os.path.join(ROOT, "tests", "golden", "reference_python_calls.json")) as f:
        calls = json.dumps(json.load(f))
    for n in PYNI:
        assert '"%s"' % n in calls, n


def test_pyni_exports_the_new_names():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host")], check=True)
    code = "import pyniNVStrings as P; print(' '.join(n for n in %r if not hasattr(P, n)))" % PYNI
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "custrings_amd") + os.pathsep + ROOT)
    out = subprocess.run(["python3", "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == ""


def test_python_api_no_longer_refuses_them():
    import nvstrings as top
    from custrings_amd import nvstrings as N

    for n in m.MEMBERS:
        assert n not in N._NOT_BUILT and callable(getattr(N.nvstrings, n)) and callable(getattr(top.nvstrings, n)), n
    for n in ("compare", "find_from", "rfind", "match_strings", "startswith", "endswith", "find_multiple", "get_ipc_data"):
        assert n not in N._NOT_BUILT and callable(getattr(N.nvstrings, n)), n  # (long built: no dead entries)
    assert set(N._NOT_BUILT) == {"fillna", "index", "rindex", "translate", "url_encode", "url_decode"}
