"""The substring / padding / wrapping ops without a GPU: the Python model (tests/pad_model.py) against the reference's
known answers; pad_ops.h (the text the kernels compile) built with g++ against the model on about 1M generated rows; the
relink of the twelve NVStrings members; the pyni names the reference's Python layer calls."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cpulibs
import pad_model as m

ROOT = cpulibs.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_pad.json")
MEMBERS = ["get", "slice", "slice_from", "slice_replace", "insert", "repeat", "pad", "ljust", "rjust", "center", "zfill", "wrap"]


def cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def _model(case):
    rows = case["input"]
    if case["op"] == "slice_from":
        a = list(case["args"]) + [None, None]
        starts = case["kwargs"].get("starts", a[0])
        stops = case["kwargs"].get("stops", a[1])
        return [m.apply("slice_from", r, None, (0 if starts is None else starts[i], -1 if stops is None else stops[i]))
                for i, r in enumerate(rows)]
    return [m.apply(case["op"], r, m.member_args(case["op"], case["args"], case["api"])) for r in rows]


def test_golden_covers_every_member():
    assert {c["op"] for c in cases()} == set(MEMBERS)
    assert {c["src"].split(":")[0] for c in cases()} == {"cpp/tests/test_pad.cpp", "cpp/tests/test_modify.cu", "python/tests/test_pad.py",
                                                          "python/tests/test_substr.py", "python/tests/test_wrap.py"}


@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s-%s" % (c["op"], c["src"].split(":")[-1], c["args"]))
def test_model_reproduces_known_answers(case):
    assert _model(case) == case["expected"], case["src"]


def test_model_quirks_and_deviation():
    assert m.apply("slice", "Héllo", [2, 0]) == "llo"  # stop 0 is the end
    assert m.apply("slice", "Héllo", [-2, -1]) == ""  # a negative start is past the end
    assert m.apply("slice_replace", "Héllo", ["x", -1, -1]) == "Héllox"  # a negative start appends
    assert m.apply("slice_replace", "Héllo", ["x", 3, 1]) == "Héllo"  # a stop before the start: unchanged
    assert m.apply("slice_replace", "Héllo", ["x", 1, -1]) == "Hx"  # stop -1: the end
    assert m.apply("insert", "Héllo", ["x", 6]) == "Héllo" and m.apply("insert", "Héllo", ["x", 5]) == "Héllox"
    assert m.apply("insert", "Héllo", ["x", -7]) == "Héllox"
    assert m.apply("zfill", "thesé", [8]) == "000thesé" and m.apply("zfill", "+1", [4]) == "+001"
    assert m.apply("repeat", "ab", [0]) == "ab" and m.apply("repeat", "", [-1 & 0xFFFFFFFF]) == ""
    assert m.apply("center", "a", [4, "é"]) == "éaéé"
    assert m.apply("ljust", "a", [3, "€x"]) == "a€€"  # only the first character of fillchar
    assert m.apply("wrap", "a\tb c", [1]) == "a\nb\nc"
    # deviation 1: a strided slice over multi-byte characters takes characters, not bytes
    assert m.apply("slice", "accénted", [2, 8, 2]) == "cne"
    assert m.apply("slice", "ééééé", [0, 4, 3]) == "éé"


# ---- the harness (pad_ops.h) against the model ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


def test_harness_reproduces_known_answers(harness):
    for case in cases():
        rows = [None if r is None else r.encode() for r in case["input"]]
        want = [None if e is None else e.encode() for e in case["expected"]]
        if case["op"] == "slice_from":
            a = list(case["args"]) + [None, None]
            starts = case["kwargs"].get("starts", a[0])
            got = harness.run("slice", rows, starts=starts, stops=case["kwargs"].get("stops", a[1]))
        else:
            op, kw = m.member_kwargs(case["op"], m.member_args(case["op"], case["args"], case["api"]))
            got = harness.run(op, rows, **kw)
        assert got == want, case["src"]


ROWS = 1_000_000
SETTINGS = [
    ("slice", dict(start=2, stop=8)), ("slice", dict(start=0, stop=0)), ("slice", dict(start=-1, stop=5)),
    ("slice", dict(start=3, stop=-1, step=2)), ("slice", dict(start=1, stop=20, step=3)), ("slice", dict(start=5, stop=5)),
    ("slice_replace", dict(repl=b"_\xc3\xa9_", start=2, stop=5)), ("slice_replace", dict(repl=b"x", start=-1, stop=-1)),
    ("slice_replace", dict(repl=b"", start=4, stop=1)), ("slice_replace", dict(repl=b"zz", start=23, stop=-1)),
    ("insert", dict(repl=b"**", start=1)), ("insert", dict(repl=b"+", start=-1)), ("insert", dict(repl=b"\xe2\x82\xac", start=12)),
    ("repeat", dict(reps=0)), ("repeat", dict(reps=3)), ("ljust", dict(width=12)), ("rjust", dict(width=24, fill=b"\xc3\xa9")),
    ("center", dict(width=13, fill=b"_")), ("center", dict(width=0)), ("zfill", dict(width=10)), ("wrap", dict(width=4)),
    ("wrap", dict(width=0)), ("wrap", dict(width=9)),
]


@pytest.fixture(scope="module")
def generated():
    return m.gen_rows(ROWS // len(SETTINGS) + 1, seed=3)


@pytest.mark.parametrize("k", range(len(SETTINGS)), ids=lambda k: "%s-%d" % (SETTINGS[k][0], k))
def test_harness_matches_model_on_generated_rows(harness, generated, k):
    op, kw = SETTINGS[k]
    rows = generated
    got = harness.run(op, rows, **kw)
    args = {"slice": lambda: [kw["start"], kw["stop"], kw.get("step", 1)],
            "slice_replace": lambda: [kw["repl"].decode(), kw["start"], kw["stop"]],
            "insert": lambda: [kw["repl"].decode(), kw["start"]],
            "repeat": lambda: [kw["reps"]]}.get(op, lambda: [kw["width"]] + ([kw["fill"].decode()] if "fill" in kw else []))()
    want = m.apply_column(op, rows, args)
    bad = [i for i in range(len(rows)) if got[i] != want[i]]
    assert not bad, [(rows[i], got[i], want[i]) for i in bad[:5]]


def test_harness_slice_from_matches_model(harness, generated):
    rng = np.random.default_rng(5)
    n = len(generated)
    starts = rng.integers(-3, 30, size=n).astype(np.int32)
    stops = rng.integers(-3, 30, size=n).astype(np.int32)
    for s, e in ((starts, stops), (starts, None), (None, stops)):
        got = harness.run("slice", generated, starts=s, stops=e)
        assert got == m.apply_column("slice_from", generated, None, s, e)


def test_harness_oversize_rows(harness):
    rows = [b"ab", b"", None, "é".encode() * 3]
    assert harness.run("repeat", rows, reps=0xFFFFFFFF) == ["RANGE", b"", None, "RANGE"]
    assert harness.run("ljust", rows, width=0x80000000) == ["RANGE", "RANGE", None, "RANGE"]


# ---- relink: a caller of the twelve members, compiled against the reference's headers ---------------------------------------
CALLER = r"""
#include "NVStrings.h"
void calls(NVStrings* s, const int* st, const int* sp) {
  s->get(1); s->slice(0, 2, 1); s->slice_from(st, sp); s->slice_replace("x", 1, 2); s->insert("x", 1); s->repeat(2);
  s->pad(5, NVStrings::both, "_"); s->ljust(5); s->rjust(5); s->center(5); s->zfill(5); s->wrap(5);
}
"""
REF_INCLUDE = "/root/reference/cpp/include"
SYMBOLS = os.path.join(ROOT, "tests", "golden", "relink_pad_symbols.json")


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
    assert len(wanted) == 12
    if not os.path.isdir(REF_INCLUDE):
        pytest.skip("the reference headers are not on this machine")
    assert caller_symbols(REF_INCLUDE) == wanted


def test_our_headers_give_the_recorded_symbols():
    with open(SYMBOLS) as f:
        wanted = json.load(f)["symbols"]
    assert caller_symbols(os.path.join(ROOT, "include", "nvstrings")) == wanted


def test_pad_members_relink_against_libnvstrings():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host"), "libs"], check=True)
    with open(SYMBOLS) as f:
        wanted = set(json.load(f)["symbols"])
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "custrings_amd", "libNVStrings.so")],
                         capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not (wanted - have), sorted(wanted - have)


# ---- the pyni glue names ---------------------------------------------------------------------------------------------------
PYNI = ["n_get", "n_slice", "n_slice_from", "n_slice_replace", "n_insert", "n_repeat", "n_pad", "n_ljust", "n_center", "n_rjust",
        "n_zfill", "n_wrap"]


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
    from custrings_amd import nvstrings as N

    for n in MEMBERS:
        assert n not in N._NOT_BUILT and callable(getattr(N.nvstrings, n)), n
