"""url_encode / url_decode / translate / fillna / index / rindex without a GPU: the Python model (tests/recode_model.py)
against the reference's known answers and the documented quirks; recode_ops.h (the text the kernels compile) built with g++
and the address / undefined-behaviour sanitizers, run as a child process, against the model on about 1M generated rows; the
relink of the five NVStrings members; the pyni names the reference's Python layer calls; the public API."""
import json
import os
import subprocess
import tempfile
import urllib.parse

import pytest

import cpulibs
import recode_model as m

ROOT = cpulibs.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_recode.json")
METHODS = ["url_encode", "url_decode", "translate", "fillna", "index", "rindex"]


def cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_golden_covers_every_method():
    assert {c["op"] for c in cases()} == set(METHODS)
    assert {c["src"].split(":")[0] for c in cases()} == {"cpp/tests/test_url.cpp", "cpp/tests/test_modify.cu", "python/tests/test_url.py",
                                                          "python/tests/test_translate.py", "python/tests/test_substr.py",
                                                          "python/tests/test_compare.py"}
    have = {c["src"] for c in cases()}
    for src in ("cpp/tests/test_modify.cu:79", "cpp/tests/test_modify.cu:87", "cpp/tests/test_modify.cu:125", "python/tests/test_compare.py:109",
                "python/tests/test_compare.py:118"):
        assert src in have, src


@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s-%s" % (c["op"], c["src"].split("/")[-1], c.get("table", "")))
def test_model_reproduces_known_answers(case):
    assert m.apply_case(case) == case["expected"], case["src"]


def test_unreserved_set_is_pythons_over_all_ascii():
    for c in range(128):
        kept = urllib.parse.quote(bytes([c]), safe="") == chr(c)
        assert kept == (c in m.UNRESERVED), c
        assert m.encode_row(bytes([c])) == (bytes([c]) if c in m.UNRESERVED else b"%%%02X" % c)
    assert m.encode_row("é€".encode()) == b"%C3%A9%E2%82%AC"
    assert m.encode_row(b"\xff\x80a") == b"%FF%80a"  # (not valid UTF-8: the byte rule)


def test_decode_quirks():
    assert m.decode_row(b"%41") == b"A"
    assert m.decode_row(b"%4") == b"%4"
    assert m.decode_row(b"a%") == b"a%"
    assert m.decode_row(b"%%41") == b"\x041"  # the first '%' consumes "%4"
    assert m.decode_row(b"%zz") == b"\x53"  # z = 122 - 87 = 35: (35 * 16) % 256 + 35 = 48 + 35
    assert m.decode_row(b"%%%") == b"\x00"  # "%%" are two digits of value 0
    assert m.decode_row(b"%GG") == bytes([(16 * 16) % 256 + 16])  # all of A-Z count: G = 16
    assert m.decode_row(b"%c3%a9") == "é".encode()


def test_decode_agrees_with_urllib_on_well_formed_escapes():
    rows = [r for r in m.gen_rows(20000, seed=11) if r is not None]
    import re
    good = [r for r in rows if all(re.match(rb"[0-9A-Fa-f]{2}", r[i + 1:i + 3]) and i + 2 < len(r) for i in range(len(r)) if r[i] == 0x25)]
    good += [b"a%20b", b"%C3%A9%e2%82%ac", b"%00%ff", b"%25%32%35", b"", b"no escapes"]
    assert len(good) > 1000
    for r in good:
        assert m.decode_row(r) == urllib.parse.unquote_to_bytes(r), r


def test_translate_quirks():
    t = m.translate_row
    assert t("hello wörld".encode(), [[ord("l"), 0]]) == "heo wörd".encode()  # delete
    assert t(b"a-b", [[ord("-"), 0x20AC]]) == "a€b".encode()  # 1 -> 3 bytes
    assert t("héé".encode(), [[0xE9, ord("e")]]) == b"hee"  # 2 -> 1 byte
    assert t(b"abc", [[ord("a"), ord("x")], [ord("a"), ord("y")]]) == b"ybc"  # a duplicate key: the last pair wins
    assert t("ééa".encode(), [[0xE9, ord("1")], [0xE9, 0]]) == b"a"
    assert t(b"ab", [[ord("a"), ord("b")], [ord("b"), ord("c")]]) == b"bc"  # looked up once, the result not again
    assert t(b"a\x00b", [[0, ord("0")]]) == b"a0b"  # key 0 is the NUL byte
    assert t("😀x".encode(), [[0x1F600, ord("!")]]) == b"!x"
    # not valid UTF-8: a malformed sequence matches no key and is copied
    assert t(b"\xa9a\xc3", [[0xE9, ord("e")], [ord("a"), ord("b")]]) == b"\xa9b\xc3"
    assert t(b"\xc0\x80", [[0, ord("0")]]) == b"\xc0\x80"  # an over-long NUL is not key 0
    assert t(b"a\xed\xa0\x80", [[0xD800, ord("x")], [ord("a"), ord("b")]]) == b"b\xed\xa0\x80"  # an encoded surrogate is no character
    assert t(b"\xc3A", [[ord("A"), ord("B")], [0xC1, ord("x")]]) == b"\xc3A"  # the lead byte takes its two bytes, broken as they are


# ---- the harness (recode_ops.h) against the model --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


BIG_TABLE = [[0x100 + k, (0x20AC if k % 3 == 0 else ord("a") + k % 26 if k % 3 == 1 else 0)] for k in range(300)]
TABLES = {
    "empty": [],
    "ascii": [[ord("a"), ord("A")], [ord("%"), 0], [ord(" "), ord("_")], [0, ord("0")], [0x7F, ord("?")], [0xD800, ord("x")], [0xD802, 0]],
    "widths": [[ord("-"), 0x20AC], [0xE9, ord("e")], [0x20AC, 0x1F600], [0x1F600, 0xDF], [0x4E2D, 0], [ord("b"), 0xF1]],
    "duplicates": [[ord("a"), ord("x")], [0xE9, ord("1")], [ord("a"), ord("y")], [0xE9, 0x4E2D], [0xE9, 0x20AC]],
    "delete-all": [[ord(c), 0] for c in set("".join(m.ALPHABET))],
    "300-keys": BIG_TABLE + [[0xE9, 0x1F600], [ord("Z"), 0xE9]],
}
ROWS = 1_000_000
SETTINGS = [("url_encode", None), ("url_decode", None)] + [("translate", k) for k in TABLES]


def test_harness_reproduces_known_answers(harness):
    for case in cases():
        if case["op"] not in m.OPS:
            continue
        rows = [None if r is None else r.encode() for r in case["input"]]
        want = [None if e is None else e.encode() for e in case["expected"]]
        assert harness.run(case["op"], rows, case["args"]) == want, case["src"]


@pytest.fixture(scope="module")
def generated():
    n = ROWS // len(SETTINGS)
    return m.gen_rows(n - n // 8, seed=3) + m.gen_byte_rows(n // 8, seed=4) + m.percent_tail_rows()


@pytest.mark.parametrize("k", range(len(SETTINGS)), ids=lambda k: "%s-%s" % SETTINGS[k])
def test_harness_matches_model_on_generated_rows(harness, generated, k):
    op, table = SETTINGS[k]
    pairs = TABLES[table] if table else None
    got = harness.run(op, generated, pairs)  # (sizes against bytes written: the harness's own exit code)
    want = m.apply_column(op, generated, pairs)
    bad = [i for i in range(len(generated)) if got[i] != want[i]]
    assert not bad, [(generated[i], got[i], want[i]) for i in bad[:5]]


def test_harness_refuses_a_code_point_beyond_unicode(harness):
    with pytest.raises(AssertionError, match=r"^\(4,"):
        harness.run("translate", [b"a"], [[ord("a"), 0x110000]])
    with pytest.raises(AssertionError, match=r"^\(4,"):
        harness.run("translate", [b"a"], [[0x110000, ord("a")]])


# ---- relink: a caller of the five members, compiled against the reference's headers ----------------------------------------
CALLER = r"""
#include "NVStrings.h"
void calls(NVStrings* s, NVStrings& o, std::pair<unsigned, unsigned>* t) {
  s->translate(t, 2); s->fillna("x"); s->fillna(o); s->url_encode(); s->url_decode();
}
"""
REF_INCLUDE = "/root/reference/cpp/include"
SYMBOLS = os.path.join(ROOT, "tests", "golden", "relink_recode_symbols.json")


def caller_symbols(include_dir):
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "caller.cpp"), os.path.join(d, "caller.o")
        open(src, "w").write(CALLER)
        subprocess.run(["g++", "-std=c++14", "-c", "-I", include_dir, src, "-o", obj], check=True)
        out = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
        return sorted({ln.split()[-1] for ln in out.splitlines() if "NVStrings" in ln})


def test_recorded_symbols_match_reference_headers():
    with open(SYMBOLS) as f:
        wanted = json.load(f)["symbols"]
    assert len(wanted) == 5
    if not os.path.isdir(REF_INCLUDE):
        pytest.skip("the reference headers are not on this machine")
    assert caller_symbols(REF_INCLUDE) == wanted


def test_our_headers_give_the_recorded_symbols():
    with open(SYMBOLS) as f:
        wanted = json.load(f)["symbols"]
    assert caller_symbols(os.path.join(ROOT, "include", "nvstrings")) == wanted


def test_recode_members_relink_against_libnvstrings():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host"), "libs"], check=True)
    with open(SYMBOLS) as f:
        wanted = set(json.load(f)["symbols"])
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "custrings_amd", "libNVStrings.so")],
                         capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not (wanted - have), sorted(wanted - have)


# ---- the pyni glue names and the public API ---------------------------------------------------------------------------------
PYNI = ["n_" + n for n in METHODS]


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


def test_c_abi_declares_the_entry_points():
    from custrings_amd import _lib

    for n in ("cs_url_encode", "cs_url_decode", "cs_translate", "cs_fillna", "cs_fillna_column"):
        assert n in _lib._PROTOS and hasattr(_lib.lib, n), n


def test_python_api_has_all_six():
    import sys

    from custrings_amd import nvstrings as N

    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import nvstrings as top

    for n in METHODS:
        assert callable(N.nvstrings.__dict__[n]), n  # (defined on the class: __getattr__ and _NOT_BUILT are never asked)
        assert callable(getattr(top.nvstrings, n)), n
