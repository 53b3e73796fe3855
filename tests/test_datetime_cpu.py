"""The timestamp conversions without a GPU: the Python model (tests/datetime_model.py) against the reference's known
answers and, independently, against numpy.datetime64; datetime_ops.h (the text the kernels compile) built with g++
against the model on generated inputs; the format compiler's errors; the relink of the two NVStrings members."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cpulibs
import datetime_model as m

ROOT = cpulibs.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_datetime.json")


def cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def _fmt(case):
    return None if case["format"] is None else case["format"].encode()


def test_golden_covers_both_ops():
    assert {c["op"] for c in cases()} == {"timestamp2long", "long2timestamp"}
    assert {c["src"].split(":")[0] for c in cases()} == {"cpp/tests/test_datetime.cu", "python/tests/test_datetime.py",
                                                          "python/nvstrings.py"}


@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s" % (c["op"], c["src"].split(":")[-1]))
def test_model_reproduces_known_answers(case):
    units = m.UNITS[case["units"]]
    if case["op"] == "timestamp2long":
        rows = [None if s is None else s.encode() for s in case["input"]]
        got = m.parse_column(rows, _fmt(case), units)
        assert got.tolist() == case["expected"], case["src"]
        assert int((got != 0).sum()) == case["count"]
    else:
        got = m.format_column(np.array(case["input"], dtype=np.int64), None, _fmt(case), units)
        assert [g.decode() for g in got] == case["expected"], case["src"]


def test_model_quirks_and_deviations():
    items = m.compile_format(None, m.SECONDS)
    assert m.parse(b"2019-03-20", items, m.SECONDS) == 1553040000  # deviation 1: past the end reads NUL (midnight)
    assert m.parse(b"2019-03-20T12:34:56Q", items, m.SECONDS) == 1553085296  # a literal is never checked
    utc = m.compile_format(b"%Y-%m-%dT%H:%M:%S%Z", m.SECONDS)
    assert m.parse(b"2019-03-20T12:34:56UTQ", utc, m.SECONDS) == 0  # %Z must be UTC
    assert m.parse(b"2019-03-20T12:34:56utc", utc, m.SECONDS) == 1553085296
    # (no %Y: the year is 0, so these compare against the start of the day)
    ms = m.compile_format(b"%H:%M:%S.%f", m.MS)
    day0 = m.parse(b"00:00:00.000", ms, m.MS)
    assert m.parse(b"00:00:01.5Z ", ms, m.MS) - day0 == 1005  # "5" under %f is 5 ms
    assert m.parse(b"00:00:01.5", ms, m.MS) == 0  # too short for %f: the row fails
    pm = m.compile_format(b"%I %p", m.HOURS)
    h0 = m.parse(b"00 AM", pm, m.HOURS)
    assert m.parse(b"12 PM", pm, m.HOURS) - h0 == 24  # 12 PM is hour 24
    assert m.parse(b"01 pm", pm, m.HOURS) - h0 == 13
    z = m.compile_format(b"%H:%M%z", m.MINUTES)
    assert m.parse(b"10:00-0130", z, m.MINUTES) - m.parse(b"00:00+0000", z, m.MINUTES) == 600 - 90  # the offset is added
    hz = m.parse_column([b"10:00+0130", b"00:00+0000"], b"%H:%M%z", m.HOURS)
    assert hz[0] - hz[1] == 10 + 1
    assert m.parse(b"2019 x", m.compile_format(b"%Y %a", m.DAYS), m.DAYS) == 0
    fmt = m.compile_format(b"%Y|%y|%I%p|%z|%j", m.SECONDS)
    assert m.format_value(-1, fmt, m.SECONDS) == b"1970|70|00AM||001"  # days truncate toward zero; %j is the day of the month
    assert m.format_value(12345 - 1970, m.compile_format(b"%Y", m.YEARS), m.YEARS) == b"2345"  # the low digits
    assert m.format_value(-3600, m.compile_format(b"%H", m.SECONDS), m.SECONDS) == b"00"  # negative hour
    assert m.format_value(2 ** 63 - 1, m.compile_format(None, m.NS), m.NS) == b"2262-04-11T23:47:16Z"
    assert m.out_width(None, m.SECONDS) == 20 and m.out_width(b"%z%a%%", m.SECONDS) == 1


# ---- independently of the reference: numpy.datetime64 -------------------------------------------------------------------------
NP_UNIT = {"Y": "Y", "M": "M", "D": "D", "h": "h", "m": "m", "s": "s", "ms": "ms", "us": "us", "ns": "ns"}


def _datetimes(n, seed, lo="1970-01-01", hi="9999-12-31"):
    rng = np.random.default_rng(seed)
    a, b = np.datetime64(lo, "s").astype(np.int64), np.datetime64(hi + "T23:59:59", "s").astype(np.int64)
    s = rng.integers(a, b, size=n, endpoint=True)
    sub = rng.integers(0, 10**9, size=n)
    return s, sub


@pytest.mark.parametrize("unit", list(m.UNITS))
def test_model_agrees_with_numpy(unit):
    u = m.UNITS[unit]
    hi = "2262-04-10" if unit == "ns" else "9999-12-31"
    secs, sub = _datetimes(3000, seed=u, hi=hi)
    ns = secs.astype(object) * 10**9 + sub.astype(object)
    t = np.array([np.datetime64(int(x), "ns") if unit == "ns" else np.datetime64(int(s), "s") + np.timedelta64(int(f) // 1000, "us")
                  for x, s, f in zip(ns, secs, sub)])
    want = t.astype("datetime64[%s]" % NP_UNIT[unit]).astype(np.int64)
    iso = np.datetime_as_string(t, unit="ns" if unit == "ns" else "us")  # YYYY-MM-DDTHH:MM:SS.ffffff[fff]
    fw = {"ms": 3, "ns": 9}.get(unit, 6)
    for fmt, text in (
        (None, [s[:19] + "Z" for s in iso]),
        (b"%Y-%m-%d", [s[:10] for s in iso]),
        (b"%Y-%m-%dT%H:%M:%S.%fZ", [s[:20] + s[20:20 + fw] + "Z" for s in iso]),
    ):
        got = m.parse_column([x.encode() for x in text], fmt, u)
        keep = want if fmt != b"%Y-%m-%d" else t.astype("datetime64[D]").astype("datetime64[%s]" % NP_UNIT[unit]).astype(np.int64)
        if unit in ("us", "ns") and fmt != b"%Y-%m-%dT%H:%M:%S.%fZ":
            keep = t.astype("datetime64[s]" if fmt is None else "datetime64[D]").astype("datetime64[%s]" % unit).astype(np.int64)
        elif unit == "ms" and fmt is None:
            keep = t.astype("datetime64[s]").astype("datetime64[ms]").astype(np.int64)
        assert np.array_equal(got, keep), (unit, fmt)
    # 12-hour clock, two-digit years (1900-1999), hours other than 0 and 12 (the reference's %p quirk)
    s20, _ = _datetimes(3000, seed=100 + u, lo="1900-01-01", hi="1999-12-31")
    t20 = s20.astype("datetime64[s]")
    hours = (s20 // 3600) % 24
    ok = (hours % 12) != 0
    t20 = t20[ok].astype("datetime64[m]")
    text = []
    for x in t20.astype(object):
        text.append("%02d/%02d/%02d %02d:%02d %s" % (x.month, x.day, x.year % 100, x.hour % 12, x.minute, "PM" if x.hour >= 12 else "AM"))
    got = m.parse_column([x.encode() for x in text], b"%m/%d/%y %I:%M %p", u)
    assert np.array_equal(got, t20.astype("datetime64[%s]" % NP_UNIT[unit]).astype(np.int64)), unit
    # format: the value in the unit back to ISO text
    vals = want
    got = m.format_column(vals, None, b"%Y-%m-%dT%H:%M:%S.%fZ", u)
    back = np.datetime_as_string(vals.astype("datetime64[%s]" % NP_UNIT[unit]).astype("datetime64[%s]" % ("ns" if unit == "ns" else "us")),
                                 unit="ns" if unit == "ns" else "us")
    assert [g.decode() for g in got] == [s[:20] + s[20:20 + fw] + "Z" for s in back], unit


# ---- the harness (datetime_ops.h) against the model ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


PARSE_ROWS = 90_000  # x 11 formats: about 1M rows
FORMAT_VALUES = 110_000  # x 9 units: about 1M values


@pytest.mark.parametrize("fi", range(len(m.FORMATS)), ids=lambda i: "fmt%d" % i)
def test_harness_matches_model_on_generated_rows(harness, fi):
    fmt = m.FORMATS[fi]
    rows = m.gen_rows(PARSE_ROWS, seed=fi)
    units = [m.SECONDS, (fi * 2) % 9, (fi * 2 + 1) % 9]
    third = PARSE_ROWS // 3
    for k, u in enumerate(units):
        part = rows[k * third:(k + 1) * third]
        got = harness.parse(part, fmt, u)
        want = m.parse_column(part, fmt, u)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, [(part[i], int(got[i]), int(want[i])) for i in bad[:5]]


@pytest.mark.parametrize("units", list(m.UNITS))
def test_harness_matches_model_on_generated_values(harness, units):
    u = m.UNITS[units]
    vals = m.gen_values(FORMAT_VALUES, seed=u)
    fmts = [None, b"%Y-%m-%dT%H:%M:%S.%fZ", b"%y%m%d %I%p %j %z%%%a %Z", b"just text"]
    part = FORMAT_VALUES // len(fmts)
    for k, fmt in enumerate(fmts):
        v = vals[k * part:(k + 1) * part]
        got = harness.format(v, fmt, u)
        want = m.format_column(v, None, fmt, u)
        w = m.out_width(fmt, u)
        assert harness.compile(fmt, u) == (0, w)
        assert len(got) == w * len(v)
        if got != b"".join(want):
            bad = next(i for i in range(len(v)) if got[i * w:(i + 1) * w] != want[i])
            raise AssertionError((int(v[bad]), got[bad * w:(bad + 1) * w], want[bad]))


def test_format_compiler_errors(harness):
    for fmt, code in ((b"%Y-%", 1), (b"%Q", 2), (b"%", 1), (b"%Y %e", 2), (b"x" * 300, 3), (b"%Y" * 65, 3)):
        assert harness.compile(fmt, m.SECONDS)[0] == code, fmt
        if code != 3:  # (the bound of the program in the kernel arguments: the model has none)
            with pytest.raises(ValueError):
                m.compile_format(fmt, m.SECONDS)
    assert harness.compile(None, 9)[0] == 4 and harness.compile(None, -1)[0] == 4
    assert harness.compile(b"%%%Y%%", m.SECONDS) == (0, 6)
    assert harness.compile(b"", m.SECONDS) == (0, 0)


# ---- relink: a caller of the two members, compiled against the reference's headers ---------------------------------------------
CALLER = r"""
#include "NVStrings.h"
void calls(NVStrings* s, unsigned long* lp, unsigned char* m) {
  s->timestamp2long("%Y", NVStrings::seconds, lp);
  NVStrings::long2timestamp(lp, 1, NVStrings::ms, nullptr, m);
}
"""
REF_INCLUDE = "/root/reference/cpp/include"
SYMBOLS = os.path.join(ROOT, "tests", "golden", "relink_datetime_symbols.json")


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
    assert len(wanted) == 2
    if os.path.isdir(REF_INCLUDE):
        assert caller_symbols(REF_INCLUDE) == wanted
    assert caller_symbols(os.path.join(ROOT, "include", "nvstrings")) == wanted


def test_timestamp_members_relink_against_libnvstrings():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host"), "libs"], check=True)
    with open(SYMBOLS) as f:
        wanted = set(json.load(f)["symbols"])
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "custrings_amd", "libNVStrings.so")],
                         capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not (wanted - have), sorted(wanted - have)
