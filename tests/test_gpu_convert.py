"""The conversion ops on the MI355X: the reference's known answers through the Python API, the pyni glue and a C++ program
built against include/nvstrings; generated columns against the model (tests/convert_model.py) and the CPU harness of
convert_ops.h on both parse routes; the format ops byte for byte; device round trips; the headline column's fields."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import convert_model as m
import cpulibs
import gpuutil

pytestmark = pytest.mark.gpu

ROOT = cpulibs.ROOT
PARSE_OPS = ["hash", "stoi", "stol", "stof", "stod", "htoi", "ip2int", "to_bools"]
FORMAT_OPS = ["itos", "ltos", "ftos", "dtos", "int2ip", "from_bools"]
TORCH = {np.uint32: "int32", np.int32: "int32", np.int64: "int64", np.float32: "float32", np.float64: "float64", np.uint8: "uint8"}


def cases():
    with open(os.path.join(ROOT, "tests", "golden", "reference_convert.json")) as f:
        return json.load(f)["cases"]


def _lib():
    return gpuutil.lib()


def _route():
    return _lib().lib.cs_debug_last_route().decode()


def column(rows):
    """a device column from bytes / None rows"""
    from custrings_amd import nvstrings

    chars, offs, nulls = m.to_arrow(rows)
    valid = np.packbits(1 - nulls, bitorder="little")
    valid = np.concatenate([valid, np.zeros(8, dtype=np.uint8)])
    return nvstrings.from_offsets64(chars if chars.size else np.zeros(1, dtype=np.uint8), offs, len(rows), valid)


def parse_host(g, op, true=None):
    """(results, count) through the C ABI into host memory"""
    L = _lib()
    n = g.size()
    res = np.zeros(max(n, 1), dtype=m.PARSE_DTYPE[op])
    cnt = C.c_int64()
    if op == "to_bools":
        L.check(L.lib.cs_to_bools(g.m_cptr, true, res.ctypes.data, 0, None, C.byref(cnt)))
    else:
        L.check(getattr(L.lib, "cs_" + op)(g.m_cptr, res.ctypes.data, 0, None, C.byref(cnt)))
    return res[:n], cnt.value


def parse_device(g, op, true=None):
    import torch

    L = _lib()
    dt = m.PARSE_DTYPE[op]
    t = torch.zeros(g.size(), dtype=getattr(torch, TORCH[dt]), device="cuda")
    cnt = C.c_int64()
    if op == "to_bools":
        L.check(L.lib.cs_to_bools(g.m_cptr, true, t.data_ptr(), 1, None, C.byref(cnt)))
    else:
        L.check(getattr(L.lib, "cs_" + op)(g.m_cptr, t.data_ptr(), 1, None, C.byref(cnt)))
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dt), cnt.value


def exported(g):
    """list of bytes / None"""
    chars, offs, valid = g._export64()
    bits = np.unpackbits(valid, bitorder="little")[: g.size()]
    data, o = chars.tobytes(), offs.tolist()
    return [data[o[i]:o[i + 1]] if bits[i] else None for i in range(g.size())]


# ---- known answers -------------------------------------------------------------------------------------------------------
def _expect_parse(case, i, got):
    op, e = case["op"], case["expected"][i]
    if op in ("stof", "stod"):
        want = 0 if e is None else int(e, 16)
        have = int(m.bits(np.array([got], dtype=m.PARSE_DTYPE[op]))[0])
        if case.get("deviation", {}).get("row") == i:
            assert abs(have - want) == 1 and float(got) == m.stod(case["input"][i].encode())
            return
        assert have == want, (case["src"], case["input"][i], hex(have))
    elif op == "to_bools":
        assert (None if got is None else bool(got)) == (None if e is None and case["api"] == "python" else bool(e)), case["src"]
    else:
        assert (None if got is None else int(got)) == (None if e is None and case["api"] == "python" else int(e or 0)), case["src"]


def _format_values(case):
    op, vals = case["op"], case["input"]
    if op in ("ftos", "dtos"):
        vals = [m.hexbits(v, op) for v in vals]
    return np.array([0 if v is None else v for v in vals], dtype=m.FORMAT_DTYPE[op])


@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s" % (c["op"], c["src"].split(":")[-1]))
def test_known_answers_python_api(case):
    from custrings_amd import nvstrings

    op = case["op"]
    if op in FORMAT_OPS:
        fn = {"from_bools": "from_booleans"}.get(op, op)
        kw = {k: case[k] for k in ("true", "false", "nulls") if k in case}
        got = getattr(nvstrings, fn)(_format_values(case), **kw)
        assert got.to_host() == case["expected"], case["src"]
        return
    s = nvstrings.to_device(case["input"])
    if op == "to_bools":
        res = s.to_booleans(true=case.get("true", "True"))
    else:
        res = getattr(s, op)()
    for i, v in enumerate(res):
        if v is None:
            assert case["input"][i] is None
            continue
        if op in ("stof", "stod"):
            v = np.array([v], dtype=m.PARSE_DTYPE[op])[0]
        _expect_parse(case, i, v)
    # the count the C ABI returns: non-zero results (to_bools: trues)
    _, cnt = parse_host(s, op, case.get("true", "True").encode() if op == "to_bools" else None)
    want = m.parse_column(op, [None if x is None else x.encode() for x in case["input"]],
                          case.get("true", "True").encode() if op == "to_bools" else None)
    assert cnt == m.nonzero_count(want)


@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s" % (c["op"], c["src"].split(":")[-1]))
def test_known_answers_pyni_glue(case):
    import pyniNVStrings as P

    op = case["op"]
    if op in FORMAT_OPS:
        vals = _format_values(case)
        nulls = case.get("nulls")
        if op == "from_bools":
            h = P.n_createFromBools(vals.astype(np.bool_), 0, nulls, case.get("true", "True"), case.get("false", "False"), False)
        else:
            fn = {"itos": "n_createFromInt32s", "ltos": "n_createFromInt64s", "ftos": "n_createFromFloat32s",
                  "dtos": "n_createFromFloat64s", "int2ip": "n_createFromIPv4Integers"}[op]
            h = getattr(P, fn)(vals, 0, nulls, False)
        try:
            assert P.n_createHostStrings(h) == case["expected"], case["src"]
        finally:
            P.n_destroyStrings(h)
        return
    h = P.n_createFromHostStrings(case["input"])
    try:
        if op == "to_bools":
            res = P.n_to_bools(h, case.get("true", "True"), None)
        else:
            res = getattr(P, "n_" + op)(h, None)
        for i, v in enumerate(res):
            if v is None:
                assert case["input"][i] is None
                continue
            if op in ("stof", "stod"):
                v = np.array([v], dtype=m.PARSE_DTYPE[op])[0]
            _expect_parse(case, i, v)
    finally:
        P.n_destroyStrings(h)


CPP = r"""
#include <cstdio>
#include <cstring>
#include <cmath>
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
  {  // TestConvert.Hash
    const char* h[] = {"thes\xc3\xa9", nullptr, "are", "the", "t\xc3\xa9st", "strings", ""};
    NVStrings* s = NVStrings::create_from_array(h, 7);
    unsigned r[7];
    CHECK(s->hash(r, false) == 6);
    unsigned e[] = {126208335, 0, 3771471008u, 2967174367u, 1378466566, 3184694146u, 1257683291};
    for (int i = 0; i < 7; ++i) CHECK(r[i] == e[i]);
    NVStrings::destroy(s);
  }
  {  // TestConvert.ToInteger
    const char* h[] = {"1234", nullptr, "-876", "543.2", "-0.12", ".55", "-.002", "", "de", "abc123", "123abc", "456e", "-1.78e+5"};
    NVStrings* s = NVStrings::create_from_array(h, 13);
    int r[13];
    long l[13];
    int e[] = {1234, 0, -876, 543, 0, 0, 0, 0, 0, 0, 123, 456, -1};
    CHECK(s->stoi(r, false) == 6);
    CHECK(s->stol(l, false) == 6);
    for (int i = 0; i < 13; ++i) CHECK(r[i] == e[i] && l[i] == e[i]);
    CHECK(s->stoi(nullptr, false) == -1);
    NVStrings::destroy(s);
  }
  {  // TestConvert.FromInteger
    int v[] = {100, 987654321, -12761, 0, 5, -4};
    const char* e[] = {"100", "987654321", "-12761", "0", "5", "-4"};
    CHECK(same(NVStrings::itos(v, 6, nullptr, false), e, 6));
    long w[] = {100000, 9876543210L, -1276100, 0, 5, -4};
    const char* f[] = {"100000", "9876543210", "-1276100", "0", "5", "-4"};
    CHECK(same(NVStrings::ltos(w, 6, nullptr, false), f, 6));
    bool threw = false;
    try { NVStrings::itos(nullptr, 6); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
  }
  {  // TestConvert.Hex
    const char* h[] = {"1234", nullptr, "98BEEF", "1a5", "CAFE", "2face"};
    NVStrings* s = NVStrings::create_from_array(h, 6);
    unsigned r[6], e[] = {4660, 0, 10010351, 421, 51966, 195278};
    CHECK(s->htoi(r, false) == 5);
    for (int i = 0; i < 6; ++i) CHECK(r[i] == e[i]);
    NVStrings::destroy(s);
  }
  {  // TestConvert.ToFloat
    const char* h[] = {"1234", nullptr, "-876", "543.2", "-0.12", ".25", "-.002", "", "NaN", "abc123", "123abc", "456e", "-1.78e+5",
                       "-122.33644782123456789", "12e+309"};
    NVStrings* s = NVStrings::create_from_array(h, 15);
    float r[15];
    double d[15];
    float ef[] = {1234.0f, 0, -876.0f, 543.2f, -0.12f, 0.25f, -0.002f, 0, NAN, 0, 123.0f, 456.0f, -178000.0f, -122.3364486694336f, INFINITY};
    double ed[] = {1234.0, 0, -876.0, 543.2, -0.12, 0.25, -0.002, 0, NAN, 0, 123.0, 456.0, -178000.0, -122.3364478212345, INFINITY};
    CHECK(s->stof(r, false) == 12);
    CHECK(s->stod(d, false) == 12);
    for (int i = 0; i < 15; ++i) {
      CHECK(std::isnan(ef[i]) ? std::isnan(r[i]) : r[i] == ef[i]);
      CHECK(std::isnan(ed[i]) ? std::isnan(d[i]) : d[i] == ed[i]);
    }
    NVStrings::destroy(s);
  }
  {  // TestConvert.FromFloat
    float v[] = {100, 654321.25f, -12761.125f, 0, 5, -4, NAN};
    const char* e[] = {"100.0", "654321.25", "-12761.125", "0.0", "5.0", "-4.0", "NaN"};
    CHECK(same(NVStrings::ftos(v, 7, nullptr, false), e, 7));
    double w[] = {0.0000012345, 65432125000, -12761.125, 0, 5, -4, INFINITY};
    const char* f[] = {"1.2345e-06", "6.5432125e+10", "-12761.125", "0.0", "5.0", "-4.0", "Inf"};
    CHECK(same(NVStrings::dtos(w, 7, nullptr, false), f, 7));
  }
  {  // TestConvert.ToBool
    const char* h[] = {"false", nullptr, "", "true", "True", "False"};
    NVStrings* s = NVStrings::create_from_array(h, 6);
    bool r[6], e[] = {false, false, false, true, false, false};
    CHECK(s->to_bools(r, "true", false) == 1);
    for (int i = 0; i < 6; ++i) CHECK(r[i] == e[i]);
    CHECK(s->to_bools(r, nullptr, false) == 1);  // only the null row
    NVStrings::destroy(s);
  }
  {  // TestConvert.FromBool
    bool v[] = {true, false, false, true, true, true};
    const char* e[] = {"true", "false", "false", "true", "true", "true"};
    CHECK(same(NVStrings::create_from_bools(v, 6, "true", "false", nullptr, false), e, 6));
  }
  {  // TestConvert.ToIPv4
    const char* h[] = {nullptr, "", "hello", "41.168.0.1", "127.0.0.1", "41.197.0.1"};
    NVStrings* s = NVStrings::create_from_array(h, 6);
    unsigned r[6], e[] = {0, 0, 0, 698875905, 2130706433, 700776449};
    CHECK(s->ip2int(r, false) == 3);
    for (int i = 0; i < 6; ++i) CHECK(r[i] == e[i]);
    NVStrings::destroy(s);
  }
  {  // TestConvert.FromIPv4
    unsigned v[] = {3232235521u, 167772161, 0, 0, 700055553, 700776449};
    const char* e[] = {"192.168.0.1", "10.0.0.1", "0.0.0.0", "0.0.0.0", "41.186.0.1", "41.197.0.1"};
    CHECK(same(NVStrings::int2ip(v, 6, nullptr, false), e, 6));
  }
  if (bad) return 1;
  printf("convert host-API known answers passed\n");
  return 0;
}
"""


def test_known_answers_cpp_program():
    lib = os.path.join(ROOT, "custrings_amd")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "convert_kat.cpp"), os.path.join(d, "convert_kat")
        open(src, "w").write(CPP)
        subprocess.run(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", lib, "-lNVStrings",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "known answers passed" in out.stdout


# ---- differential: generated columns against the model and the harness ------------------------------------------------------
ROWS = 1 << 20
MODEL_ROWS = 60_000  # the Python model checks a slice; the harness (convert_ops.h, checked against the model) every row


@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


@pytest.fixture(scope="module")
def generated():
    rows = m.gen_rows(ROWS, seed=7)
    long_rows = m.gen_rows(4096, seed=8)
    for i in range(0, 4096, 97):  # rows over 8 KB: no tile size fits
        long_rows[i] = b"12345" * 1700 + (long_rows[i] or b"")
    return {"short": (rows, column(rows)), "long": (long_rows, column(long_rows))}


@pytest.mark.parametrize("rowwise", [False, True], ids=["default", "rowwise"])
@pytest.mark.parametrize("op", PARSE_OPS)
def test_parse_against_model(generated, harness, monkeypatch, op, rowwise):
    if rowwise:
        monkeypatch.setenv("CS_CONVERT_ROWWISE", "1")
    for which, (rows, g) in generated.items():
        for true in ([b"True", None] if op == "to_bools" else [None]):
            got, cnt = parse_host(g, op, true)
            route = _route()
            assert route == ("rows" if rowwise or which == "long" else "tile"), (which, route)
            chars, offs, nulls = m.to_arrow(rows)
            want = harness.parse(op, chars, offs, nulls, true)
            bad = np.nonzero(m.bits(got) != m.bits(want))[0]
            assert bad.size == 0, [(rows[i], got[i], want[i]) for i in bad[:5]]
            assert cnt == m.nonzero_count(want)
            sl = slice(0, min(MODEL_ROWS, len(rows)))
            assert np.array_equal(m.bits(got[sl]), m.bits(m.parse_column(op, rows[sl], true)))
            dev, dcnt = parse_device(g, op, true)
            assert np.array_equal(m.bits(dev), m.bits(got)) and dcnt == cnt


def test_parse_empty_column_and_null_output():
    L = _lib()
    g = column([])
    cnt = C.c_int64(7)
    res = np.zeros(4, dtype=np.int32)
    L.check(L.lib.cs_stoi(g.m_cptr, res.ctypes.data, 0, None, C.byref(cnt)))
    assert cnt.value == -1
    g2 = column([b"1"])
    L.check(L.lib.cs_stoi(g2.m_cptr, None, 0, None, C.byref(cnt)))
    assert cnt.value == -1
    assert g.stoi() == []


@pytest.mark.parametrize("with_nulls", [False, True], ids=["valid", "nulls"])
@pytest.mark.parametrize("op", FORMAT_OPS)
def test_format_against_model(harness, op, with_nulls):
    from custrings_amd import nvstrings

    n = 300_000
    vals = m.gen_values(op, n, seed=11 + len(op))
    nulls = np.random.default_rng(3).integers(0, 256, size=(n + 7) // 8, dtype=np.uint8) if with_nulls else None
    fn = {"from_bools": "from_booleans"}.get(op, op)
    kw = {"true": "yes", "false": ""} if op == "from_bools" else {}
    g = getattr(nvstrings, fn)(vals, nulls=nulls, **kw)
    chars, offs, valid = g._export64()
    lens, hchars = harness.format(op, vals, b"yes", b"")
    ok = np.ones(n, dtype=bool) if nulls is None else np.unpackbits(nulls, bitorder="little")[:n].astype(bool)
    want_lens = np.where(ok, lens, 0).astype(np.int64)
    want_offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(want_lens, out=want_offs[1:])
    assert np.array_equal(offs, want_offs)
    hoffs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens.astype(np.int64), out=hoffs[1:])
    hc = np.frombuffer(hchars, dtype=np.uint8)
    keep = np.repeat(ok, lens)
    assert np.array_equal(chars, hc[keep])
    assert np.array_equal(np.unpackbits(valid, bitorder="little")[:n].astype(bool), ok)
    sl = 20_000
    model = m.format_column(op, vals[:sl], nulls, b"yes", b"")
    assert exported(g.sublist(0, sl)) == model
    width = int(_lib().lib.cs_column_offset_width(g.m_cptr))
    assert width == 4  # (rows x the op's widest row < 2^31)


def test_format_invalid_arguments():
    from custrings_amd import nvstrings

    with pytest.raises(Exception):
        nvstrings.itos([])
    L = _lib()
    out = C.c_void_p()
    assert L.lib.cs_itos(None, 5, None, 0, None, C.byref(out)) == L.CS_ERR_INVALID_ARG
    v = np.zeros(3, dtype=np.uint8)
    assert L.lib.cs_from_bools(v.ctypes.data, 3, None, b"f", None, 0, None, C.byref(out)) == L.CS_ERR_INVALID_ARG


# ---- round trips on the device ---------------------------------------------------------------------------------------------
def _roundtrip(fmt, parse, tdtype, n, seed):
    import torch

    L = _lib()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    info = torch.iinfo(tdtype)
    x = torch.randint(info.min, info.max, (n,), dtype=tdtype, device="cuda", generator=gen)
    x[:3] = torch.tensor([0, info.min, info.max], dtype=tdtype)
    out = C.c_void_p()
    torch.cuda.synchronize()
    L.check(getattr(L.lib, fmt)(x.data_ptr(), n, None, 1, None, C.byref(out)))
    from custrings_amd import nvstrings

    g = nvstrings.nvstrings(out.value)
    y = torch.empty_like(x)
    cnt = C.c_int64()
    L.check(getattr(L.lib, parse)(g.m_cptr, y.data_ptr(), 1, None, C.byref(cnt)))
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    assert cnt.value == int((x != 0).sum())
    width = int(L.lib.cs_column_offset_width(g.m_cptr))
    nbytes = int(L.lib.cs_column_nbytes(g.m_cptr))
    del g
    return width, nbytes


def test_roundtrip_stoi_itos():
    import torch

    w, nb = _roundtrip("cs_itos", "cs_stoi", torch.int32, 100_000_000, 1)
    assert w == 4 and nb < (1 << 31)  # (100M x 11 bytes < 2^31)


def test_roundtrip_ip2int_int2ip():
    import torch

    # (uint32 values through an int32 tensor: the same bits)
    _roundtrip("cs_int2ip", "cs_ip2int", torch.int32, 100_000_000, 2)


def test_roundtrip_stol_ltos_int64_offsets():
    import torch

    w, nb = _roundtrip("cs_ltos", "cs_stol", torch.int64, 110_000_000, 3)
    assert w == 8  # 110M rows x 20 bytes >= 2^31: int64 offsets, whatever the bytes written


# ---- the headline column's fields -------------------------------------------------------------------------------------------
def test_headline_fields():
    rows = 1 << 20
    g3 = gpuutil.synth(3, 0, rows)
    cols = g3.split(" ")
    assert len(cols) >= 4
    for c in cols[:6]:
        fields = exported(c)
        for op in ("ip2int", "stoi"):
            got, cnt = parse_host(c, op)
            want = m.parse_column(op, fields)
            assert np.array_equal(got, want), op
            assert cnt == m.nonzero_count(want)
    # the IP field where a row holds one (C3: "<METHOD> /<path> <ip> ...": the third field)
    ips, _ = parse_host(cols[2], "ip2int")
    assert (ips != 0).mean() > 0.3
