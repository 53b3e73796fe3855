"""The timestamp conversions on the MI355X: the reference's known answers through the Python API, the pyni glue and a C++
program built against include/nvstrings; generated columns against the CPU harness of datetime_ops.h (checked against the
model by tests/test_datetime_cpu.py) on both parse routes and both format writers, in every unit; nulls, device memory,
the argument errors; a 110M-row round trip with int64 offsets."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cpulibs
import datetime_model as m
import gpuutil

pytestmark = pytest.mark.gpu

ROOT = cpulibs.ROOT


def cases():
    with open(os.path.join(ROOT, "tests", "golden", "reference_datetime.json")) as f:
        return json.load(f)["cases"]


def _lib():
    return gpuutil.lib()


def _route():
    return _lib().lib.cs_debug_last_route().decode()


def _b(fmt):
    return None if fmt is None else fmt.encode() if isinstance(fmt, str) else fmt


def column(rows):
    """a device column from bytes / None rows"""
    from custrings_amd import nvstrings

    chars, offs, nulls = m.to_arrow(rows)
    valid = np.packbits(1 - nulls, bitorder="little")
    valid = np.concatenate([valid, np.zeros(8, dtype=np.uint8)])
    return nvstrings.from_offsets64(chars if chars.size else np.zeros(1, dtype=np.uint8), offs, len(rows), valid)


def parse_host(g, fmt, units):
    L = _lib()
    res = np.zeros(max(g.size(), 1), dtype=np.int64)
    cnt = C.c_int64()
    L.check(L.lib.cs_timestamp2long(g.m_cptr, _b(fmt), units, res.ctypes.data, 0, None, C.byref(cnt)))
    return res[:g.size()], cnt.value


def parse_device(g, fmt, units):
    import torch

    L = _lib()
    t = torch.zeros(g.size(), dtype=torch.int64, device="cuda")
    cnt = C.c_int64()
    L.check(L.lib.cs_timestamp2long(g.m_cptr, _b(fmt), units, t.data_ptr(), 1, None, C.byref(cnt)))
    torch.cuda.synchronize()
    return t.cpu().numpy(), cnt.value


def exported(g):
    chars, offs, valid = g._export64()
    bits = np.unpackbits(valid, bitorder="little")[: g.size()]
    data, o = chars.tobytes(), offs.tolist()
    return [data[o[i]:o[i + 1]] if bits[i] else None for i in range(g.size())]


# ---- known answers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s" % (c["op"], c["src"].split(":")[-1]))
def test_known_answers_python_api(case):
    from custrings_amd import nvstrings

    if case["op"] == "long2timestamp":
        got = nvstrings.int2timestamp(case["input"], format=case["format"], units=case["units"])
        assert got.to_host() == case["expected"], case["src"]
        return
    s = nvstrings.to_device(case["input"])
    res = s.timestamp2int(format=case["format"], units=case["units"])
    assert res == [None if x is None else e for x, e in zip(case["input"], case["expected"])], case["src"]
    _, cnt = parse_host(s, case["format"], m.UNITS[case["units"]])
    assert cnt == case["count"]


@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s" % (c["op"], c["src"].split(":")[-1]))
def test_known_answers_pyni_glue(case):
    import pyniNVStrings as P

    if case["op"] == "long2timestamp":
        h = P.n_createFromTimestamp(np.array(case["input"], dtype=np.int64), 0, None, case["format"], case["units"], False)
        try:
            assert P.n_createHostStrings(h) == case["expected"], case["src"]
        finally:
            P.n_destroyStrings(h)
        h = P.n_createFromTimestamp(list(case["input"]), 0, None, case["format"], case["units"], False)
        P.n_destroyStrings(h)
        return
    h = P.n_createFromHostStrings(case["input"])
    try:
        res = P.n_timestamp2int(h, case["format"], case["units"], None)
        assert res == [None if x is None else e for x, e in zip(case["input"], case["expected"])], case["src"]
    finally:
        P.n_destroyStrings(h)


def test_pyni_argument_errors():
    import pyniNVStrings as P

    with pytest.raises(TypeError):
        P.n_createFromTimestamp(np.array([1.5], dtype=np.float64), 0, None, None, "s", False)
    with pytest.raises(TypeError):
        P.n_createFromTimestamp(np.array([1], dtype=np.int32), 0, None, None, "s", False)
    with pytest.raises(ValueError):
        P.n_createFromTimestamp(np.array([1], dtype=np.int64), 0, None, None, "weeks", False)
    with pytest.raises(ValueError):
        P.n_createFromTimestamp(np.array([1], dtype=np.int64), 0, None, "%Q", "s", False)
    h = P.n_createFromHostStrings(["2019-03-20T12:34:56Z"])
    try:
        with pytest.raises(ValueError):
            P.n_timestamp2int(h, None, "x", None)
        with pytest.raises(ValueError):
            P.n_timestamp2int(h, "%Y%", "s", None)
    finally:
        P.n_destroyStrings(h)


CPP = r"""
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "nvstrings/NVStrings.h"
static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
static bool same(NVStrings* s, const char** want, unsigned n) {
  std::vector<char*> rows(n);
  std::vector<std::vector<char>> bufs(n, std::vector<char>(64, 0));
  for (unsigned i = 0; i < n; ++i) rows[i] = bufs[i].data();
  s->to_host(rows.data(), 0, (int)n);
  bool ok = s->size() == n;
  for (unsigned i = 0; ok && i < n; ++i) ok = want[i] ? !strcmp(rows[i], want[i]) : true;
  NVStrings::destroy(s);
  return ok;
}
int main() {
  {  // TestTimestamp.ToTimestamp
    const char* h[] = {"1974-02-28T01:23:45Z", "2019-07-17T21:34:37Z", nullptr, ""};
    NVStrings* s = NVStrings::create_from_array(h, 4);
    unsigned long r[4];
    CHECK(s->timestamp2long("%Y-%m-%dT%H:%M:%SZ", NVStrings::seconds, r, false) == 2);
    unsigned long e[] = {131246625, 1563399277, 0, 0};
    for (int i = 0; i < 4; ++i) CHECK(r[i] == e[i]);
    CHECK(s->timestamp2long(nullptr, NVStrings::seconds, nullptr, false) == -1);
    bool threw = false;
    try { s->timestamp2long("%Y%", NVStrings::seconds, r, false); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    NVStrings::destroy(s);
    const char* d[] = {"12.28.1982", "07.17.2019"};
    s = NVStrings::create_from_array(d, 2);
    CHECK(s->timestamp2long("%m-%d-%Y", NVStrings::days, r, false) == 2);
    CHECK(r[0] == 4744 && r[1] == 18094);
    NVStrings::destroy(s);
  }
  {  // TestTimestamp.FromTimestamp
    unsigned long v[] = {1563399273};
    const char* e[] = {"07/17/2019 21:34"};
    CHECK(same(NVStrings::long2timestamp(v, 1, NVStrings::seconds, "%m/%d/%Y %H:%M", nullptr, false), e, 1));
    unsigned long w[] = {1563399273123};
    const char* f[] = {"21:34:33.123"};
    CHECK(same(NVStrings::long2timestamp(w, 1, NVStrings::ms, "%H:%M:%S.%f", nullptr, false), f, 1));
    bool threw = false;
    try { NVStrings::long2timestamp(nullptr, 1, NVStrings::ms, nullptr); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { NVStrings::long2timestamp(v, 1, NVStrings::ms, "%Q", nullptr, false); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
  }
  if (bad) return 1;
  printf("datetime host-API known answers passed\n");
  return 0;
}
"""


def test_known_answers_cpp_program():
    lib = os.path.join(ROOT, "custrings_amd")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "datetime_kat.cpp"), os.path.join(d, "datetime_kat")
        open(src, "w").write(CPP)
        subprocess.run(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", lib, "-lNVStrings",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "known answers passed" in out.stdout


# ---- differential: generated columns against the harness ---------------------------------------------------------------------
ROWS = 1 << 20
PARSE_FORMATS = [None, b"%Y-%m-%d", b"%Y-%m-%dT%H:%M:%S.%fZ", b"%m/%d/%y %I:%M %p", b"%d.%m.%Y %H:%M:%S%z", b"%j %Y %%%Z"]


@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


@pytest.fixture(scope="module")
def generated():
    rows = m.gen_rows(ROWS, seed=17)
    long_rows = m.gen_rows(4096, seed=18)
    for i in range(0, 4096, 97):  # rows over 8 KB: no tile size fits
        long_rows[i] = (long_rows[i] or b"") + b"x" * 8500
    return {"short": (rows, column(rows)), "long": (long_rows, column(long_rows))}


@pytest.mark.parametrize("rowwise", [False, True], ids=["default", "rowwise"])
@pytest.mark.parametrize("units", list(m.UNITS))
def test_parse_against_harness(generated, harness, monkeypatch, units, rowwise):
    if rowwise:
        monkeypatch.setenv("CS_CONVERT_ROWWISE", "1")
    u = m.UNITS[units]
    for which, (rows, g) in generated.items():
        for fmt in (PARSE_FORMATS if which == "short" else PARSE_FORMATS[:1]):
            got, cnt = parse_host(g, fmt, u)
            if which == "short" and fmt is None:  # (and a slice against the model itself)
                assert np.array_equal(got[:3000], m.parse_column(rows[:3000], None, u))
            assert _route() == ("rows" if rowwise or which == "long" else "tile"), which
            want = harness.parse(rows, fmt, u)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, [(rows[i], int(got[i]), int(want[i])) for i in bad[:5]]
            assert cnt == int((want != 0).sum())
        dev, dcnt = parse_device(g, None, u)
        assert np.array_equal(dev, harness.parse(rows, None, u)) and dcnt == int((dev != 0).sum())


def test_parse_empty_column_null_results_and_errors():
    L = _lib()
    cnt = C.c_int64(7)
    res = np.zeros(4, dtype=np.int64)
    g = column([])
    L.check(L.lib.cs_timestamp2long(g.m_cptr, None, 5, res.ctypes.data, 0, None, C.byref(cnt)))
    assert cnt.value == -1
    # (the empty-column and no-output checks come before the format is read)
    L.check(L.lib.cs_timestamp2long(g.m_cptr, b"%Q", 5, res.ctypes.data, 0, None, C.byref(cnt)))
    assert cnt.value == -1
    g2 = column([b"2019-03-20T12:34:56Z"])
    L.check(L.lib.cs_timestamp2long(g2.m_cptr, None, 5, None, 0, None, C.byref(cnt)))
    assert cnt.value == -1
    L.check(L.lib.cs_timestamp2long(g2.m_cptr, b"%Y", 5, None, 0, None, C.byref(cnt)))
    assert cnt.value == -1
    for fmt, units in ((b"%Y-%", 5), (b"%e", 5), (None, 9), (None, -1)):
        assert L.lib.cs_timestamp2long(g2.m_cptr, fmt, units, res.ctypes.data, 0, None, C.byref(cnt)) == L.CS_ERR_INVALID_ARG
    assert g.timestamp2int() == []
    with pytest.raises(ValueError):
        g2.timestamp2int(units="weeks")
    with pytest.raises(Exception):
        g2.timestamp2int(format="%Y%")


FORMAT_FORMATS = [None, b"%Y-%m-%dT%H:%M:%S.%fZ", b"%y%m%d %I%p %j %z%%%a %Z", b"just text"]


@pytest.mark.parametrize("rowwise", [False, True], ids=["lds", "rows"])
@pytest.mark.parametrize("units", list(m.UNITS))
def test_format_against_harness(harness, monkeypatch, units, rowwise):
    from custrings_amd import nvstrings

    if rowwise:
        monkeypatch.setenv("CS_CONVERT_ROWWISE", "1")
    u = m.UNITS[units]
    n = 300_001
    vals = m.gen_values(n, seed=30 + u)
    nulls = np.random.default_rng(u).integers(0, 256, size=(n + 7) // 8, dtype=np.uint8)
    for k, fmt in enumerate(FORMAT_FORMATS):
        w = m.out_width(fmt, u)
        hchars = np.frombuffer(harness.format(vals, fmt, u), dtype=np.uint8)
        for with_nulls in (False, True):
            nl = nulls if with_nulls else None
            g = nvstrings.int2timestamp(vals, nulls=nl, format=None if fmt is None else fmt.decode(), units=units)
            assert _route() == ("rows" if rowwise else "lds")
            chars, offs, valid = g._export64()
            ok = np.ones(n, dtype=bool) if nl is None else np.unpackbits(nl, bitorder="little")[:n].astype(bool)
            want_offs = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(np.where(ok, w, 0), out=want_offs[1:])
            assert np.array_equal(offs, want_offs), (fmt, with_nulls)
            assert np.array_equal(chars, hchars.reshape(n, w)[ok].reshape(-1) if w else chars[:0]), (fmt, with_nulls)
            assert np.array_equal(np.unpackbits(valid, bitorder="little")[:n].astype(bool), ok)
            assert int(_lib().lib.cs_column_offset_width(g.m_cptr)) == 4
        if k == 0:
            assert exported(nvstrings.int2timestamp(vals[:2000], units=units)) == m.format_column(vals[:2000], None, None, u)


def test_format_device_memory_and_errors():
    import torch

    from custrings_amd import nvstrings

    n = 100_003
    vals = m.gen_values(n, seed=5)
    nulls = np.random.default_rng(9).integers(0, 256, size=(n + 7) // 8, dtype=np.uint8)
    tv, tn = torch.from_numpy(vals).cuda(), torch.from_numpy(nulls).cuda()
    torch.cuda.synchronize()
    for units in ("s", "ms"):
        host = nvstrings.int2timestamp(vals, nulls=nulls, units=units)
        dev = nvstrings.int2timestamp(tv, nulls=tn, units=units, bdevmem=True)
        gpuutil.assert_same(dev, gpuutil.to_col(host), units)
    L = _lib()
    out = C.c_void_p()
    v = np.zeros(3, dtype=np.int64)
    assert L.lib.cs_long2timestamp(None, 3, 5, None, None, 0, None, C.byref(out)) == L.CS_ERR_INVALID_ARG
    assert L.lib.cs_long2timestamp(v.ctypes.data, 0, 5, None, None, 0, None, C.byref(out)) == L.CS_ERR_INVALID_ARG
    # (values / count are checked before the format is read: the same error either way)
    assert L.lib.cs_long2timestamp(None, 3, 5, b"%Q", None, 0, None, C.byref(out)) == L.CS_ERR_INVALID_ARG
    for fmt, units in ((b"%", 5), (b"%Q", 5), (None, 9), (None, -1)):
        assert L.lib.cs_long2timestamp(v.ctypes.data, 3, units, fmt, None, 0, None, C.byref(out)) == L.CS_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        nvstrings.int2timestamp([1], units="weeks")
    with pytest.raises(TypeError):
        nvstrings.int2timestamp(np.array([1.0]))
    # a format wider than the LDS writer takes: the per-lane writer
    wide = "%Y" + "_" * 250 + "%m%d%H%M%S"  # 264 bytes a row
    g = nvstrings.int2timestamp(vals[:5000], units="s", format=wide)
    assert _route() == "rows"
    assert exported(g) == m.format_column(vals[:5000], None, wide.encode(), m.SECONDS)


# ---- round trip on the device, int64 offsets ----------------------------------------------------------------------------------
def test_roundtrip_110m_int64_offsets():
    import torch

    from custrings_amd import nvstrings

    L = _lib()
    n = 110_000_000
    gen = torch.Generator(device="cuda").manual_seed(4)
    lo, hi = 0, 253402300799  # 1970-01-01 .. 9999-12-31 (a negative value does not round-trip: days truncate toward zero)
    x = torch.randint(lo, hi, (n,), dtype=torch.int64, device="cuda", generator=gen)
    x[:4] = torch.tensor([0, 1, hi, 1553085296], dtype=torch.int64)
    torch.cuda.synchronize()
    g = nvstrings.int2timestamp(x, units="s", bdevmem=True)
    assert int(L.lib.cs_column_offset_width(g.m_cptr)) == 8  # 110M x 20 bytes >= 2^31
    assert int(L.lib.cs_column_nbytes(g.m_cptr)) == 20 * n
    y = torch.empty_like(x)
    cnt = C.c_int64()
    L.check(L.lib.cs_timestamp2long(g.m_cptr, None, 5, y.data_ptr(), 1, None, C.byref(cnt)))
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    assert cnt.value == int((x != 0).sum())
    assert exported(g.sublist(0, 4)) == [b"1970-01-01T00:00:00Z", b"1970-01-01T00:00:01Z", b"9999-12-31T23:59:59Z",
                                         b"2019-03-20T12:34:56Z"]
