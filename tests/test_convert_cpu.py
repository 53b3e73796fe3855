"""The conversion ops without a GPU: the Python model (tests/convert_model.py) against the reference's known answers,
convert_ops.h (the text the kernels compile) built with g++ against the model on generated inputs, and the relink of
the 14 NVStrings members."""
import json
import math
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import convert_model as m
import cpulibs

ROOT = cpulibs.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_convert.json")


def cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def _rows(inp):
    return [None if s is None else s.encode() for s in inp]


def test_golden_covers_every_op():
    ops = {c["op"] for c in cases()}
    assert ops == {"hash", "stoi", "stol", "stof", "stod", "htoi", "ip2int", "to_bools", "itos", "ltos", "ftos", "dtos", "int2ip",
                   "from_bools"}
    assert sum("deviation" in c for c in cases()) == 1


@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s" % (c["op"], c["src"].split(":")[-1]))
def test_model_reproduces_known_answers(case):
    op = case["op"]
    if op in m.PARSE or op == "to_bools":
        got = m.parse_column(op, _rows(case["input"]), case.get("true", "True").encode() if op == "to_bools" else None)
        for i, e in enumerate(case["expected"]):
            if op in ("stof", "stod"):
                want = 0 if e is None else int(e, 16)
                have = int(m.bits(got[i:i + 1])[0])
                if case.get("deviation", {}).get("row") == i:
                    # P[e] scaling: the table's value, within one ulp of the reference's CUDA pow() answer
                    assert float(got[i]) == 12233644782 * m.POW10[308 - 8] * -1.0
                    assert abs(have - want) == 1
                    continue
                assert have == want, (case["src"], case["input"][i])
            else:
                assert int(got[i]) == (0 if e is None else int(e)), (case["src"], case["input"][i])
    else:
        vals = case["input"]
        if op in ("ftos", "dtos"):
            vals = [m.hexbits(v, op) for v in vals]
        vals = np.array([0 if v is None else v for v in vals], dtype=m.FORMAT_DTYPE[op])
        nulls = np.array(case["nulls"], dtype=np.uint8) if "nulls" in case else None
        got = m.format_column(op, vals, nulls, case.get("true", "True").encode(), case.get("false", "False").encode())
        assert [None if g is None else g.decode() for g in got] == case["expected"], case["src"]


def test_model_edges():
    assert m.stol(b"-9223372036854775808") == -(1 << 63)
    assert m.stol(b"18446744073709551617") == 1  # wraps
    assert m.stoi(b"4294967297") == 1
    assert m.stod(b"1e5") == 1.0  # the byte after 'e' is taken as the exponent's sign
    assert m.stod(b"1e+5") == 1e5
    assert math.isinf(m.stod(b"0e+400")) and m.stod(b"-1e-400") == 0.0 and math.copysign(1, m.stod(b"-1e-400")) == 1
    assert m.htoi(b"G") == 16 and m.htoi(b"z") == 35
    assert m.ip2int(b"1.2.3") == 0 and m.ip2int(b"1a.2.3.4") == 0x01020304 and m.ip2int(b"256.0.0.1") == 1  # (256 << 24 wraps)
    assert m.ltos(-(1 << 63)) == b"-9223372036854775808"
    assert m.dtos(-0.0) == b"0.0" and m.dtos(float("nan")) == b"NaN" and m.dtos(-float("inf")) == b"-Inf"
    assert m.dtos(9.9999999999) == b"10.0" and m.dtos(99999999999.0) == b"1.0e+11"


@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


PARSE_ROWS = 120_000  # x 8 ops
FORMAT_VALUES = 100_000  # x 6 ops: about 1.6M inputs in all


@pytest.mark.parametrize("op", ["hash", "stoi", "stol", "stof", "stod", "htoi", "ip2int", "to_bools"])
def test_harness_matches_model_on_generated_rows(harness, op):
    rows = m.gen_rows(PARSE_ROWS, seed=sum(op.encode()))
    chars, offs, nulls = m.to_arrow(rows)
    for true in ([b"True", None, b""] if op == "to_bools" else [None]):
        got = harness.parse(op, chars, offs, nulls, true)
        want = m.parse_column(op, rows, true)
        bad = np.nonzero(m.bits(got) != m.bits(want))[0]
        assert bad.size == 0, [(rows[i], got[i], want[i]) for i in bad[:5]]


@pytest.mark.parametrize("op", ["itos", "ltos", "ftos", "dtos", "int2ip", "from_bools"])
def test_harness_matches_model_on_generated_values(harness, op):
    vals = m.gen_values(op, FORMAT_VALUES, seed=len(op))
    lens, chars = harness.format(op, vals, b"yes", b"")
    want = m.format_column(op, vals, None, b"yes", b"")
    assert lens.tolist() == [len(w) for w in want]
    assert chars == b"".join(want)


# ---- relink: a caller of the 14 members, compiled against the reference's headers ------------------------------------------
CALLER = r"""
#include "NVStrings.h"
void calls(NVStrings* s, int* ip, long* lp, unsigned* up, float* fp, double* dp, bool* bp, unsigned char* m) {
  s->hash(up); s->stoi(ip); s->stol(lp); s->stof(fp); s->stod(dp); s->htoi(up); s->ip2int(up); s->to_bools(bp, "true");
  NVStrings::itos(ip, 1, m); NVStrings::ltos(lp, 1, m); NVStrings::ftos(fp, 1, m); NVStrings::dtos(dp, 1, m);
  NVStrings::int2ip(up, 1, m); NVStrings::create_from_bools(bp, 1, "t", "f", m);
}
"""
REF_INCLUDE = "/root/reference/cpp/include"
SYMBOLS = os.path.join(ROOT, "tests", "golden", "relink_convert_symbols.json")


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
    assert len(wanted) == 14
    if os.path.isdir(REF_INCLUDE):
        assert caller_symbols(REF_INCLUDE) == wanted
    # our own header declares the same members
    assert caller_symbols(os.path.join(ROOT, "include", "nvstrings")) == wanted


def test_convert_members_relink_against_libnvstrings():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host"), "libs"], check=True)
    with open(SYMBOLS) as f:
        wanted = set(json.load(f)["symbols"])
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "custrings_amd", "libNVStrings.so")],
                         capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not (wanted - have), sorted(wanted - have)
