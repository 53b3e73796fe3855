"""The character-type predicates and swapcase / capitalize / title on the MI355X: the reference's known answers through the
Python API, the pyni glue and a C++ program built against include/nvstrings; 1M-row columns against the CPU harness of
chartype_ops.h (checked against the model by tests/test_chartype_cpu.py) for all twelve ops on both routes, with the routes
asserted; counts, device / host buffers, shared extents, empty and all-null columns; one full-size check of the two routes."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import chartype_model as m
import cpulibs
import gpuutil

pytestmark = pytest.mark.gpu

ROOT = cpulibs.ROOT


def cases():
    with open(os.path.join(ROOT, "tests", "golden", "reference_chartype.json")) as f:
        return json.load(f)["cases"]


def _L():
    return gpuutil.lib()


def _route():
    return _L().lib.cs_debug_last_route().decode()


def column(rows):
    """rows of bytes / None -> a device column"""
    from custrings_amd import nvstrings

    chars, offs, nulls = m.to_arrow(rows)
    valid = np.packbits(1 - nulls, bitorder="little")
    valid = np.concatenate([valid, np.zeros(8, dtype=np.uint8)])
    return nvstrings.from_offsets64(chars if chars.size else np.zeros(1, dtype=np.uint8), offs, len(rows), valid)


def _ids(c):
    return "%s-%s" % (c["op"], c["src"].split("/")[-1])


def _api_expected(case):
    """the host list of the Python layer: None for a null row (the C++ tests' arrays hold the device's answer there)"""
    return [None if r is None else e for r, e in zip(case["input"], case["expected"])]


@pytest.mark.parametrize("case", cases(), ids=_ids)
def test_known_answers_python_api(case):
    from custrings_amd import nvstrings

    s = nvstrings.to_device(case["input"])
    got = getattr(s, case["op"])()
    if case["op"] in m.CASE_OPS:
        assert got.to_host() == case["expected"], case["src"]
        assert _route() in ("tile", "rows")
    else:
        assert got == _api_expected(case), case["src"]


@pytest.mark.parametrize("case", cases(), ids=_ids)
def test_known_answers_pyni_glue(case):
    import torch

    import pyniNVStrings as P

    h = P.n_createFromHostStrings(case["input"])
    try:
        fn = getattr(P, "n_" + case["op"])
        if case["op"] in m.CASE_OPS:
            r = fn(h)
            try:
                assert P.n_createHostStrings(r) == case["expected"], case["src"]
            finally:
                P.n_destroyStrings(r)
            return
        assert fn(h, 0) == _api_expected(case), case["src"]  # host list, None for null rows
        t = torch.full((len(case["input"]),), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert fn(h, t.data_ptr()) == t.data_ptr()
        want = [m.apply(case["op"], r) for r in case["input"]]  # (a null row on the device: False, True for is_empty)
        assert t.cpu().numpy().astype(bool).tolist() == want, case["src"]
    finally:
        P.n_destroyStrings(h)


CPP = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>
#include "nvstrings/NVStrings.h"
static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
static bool same(NVStrings* s, const char** want, unsigned n) {
  std::vector<char*> rows(n);
  std::vector<std::vector<char>> bufs(n, std::vector<char>(128, 0));
  for (unsigned i = 0; i < n; ++i) rows[i] = bufs[i].data();
  s->to_host(rows.data(), 0, (int)n);
  bool ok = s->size() == n;
  for (unsigned i = 0; ok && i < n; ++i) ok = want[i] ? !strcmp(rows[i], want[i]) : true;
  if (!ok) for (unsigned i = 0; i < n; ++i) printf("  [%u] '%s'\n", i, rows[i]);
  NVStrings::destroy(s);
  return ok;
}
#define T true
#define F false
typedef unsigned int (NVStrings::*Pred)(bool*, bool);
static void pred(NVStrings* s, Pred p, const bool* want, int line) {
  bool host[16], dev_copy[16];
  unsigned trues = 0;
  for (int i = 0; i < 16; ++i) trues += want[i];
  const unsigned n = (s->*p)(host, false);
  bool* d = nullptr;
  if (hipMalloc(&d, 16) != hipSuccess) { ++bad; return; }
  const unsigned nd = (s->*p)(d, true);
  if (hipMemcpy(dev_copy, d, 16, hipMemcpyDeviceToHost) != hipSuccess) ++bad;
  hipFree(d);
  bool ok = n == trues && nd == trues && (s->*p)(nullptr, true) == 0;
  for (int i = 0; i < 16; ++i) ok = ok && host[i] == want[i] && dev_copy[i] == want[i];
  if (!ok) { printf("FAILED predicate at line %d (count %u / %u, want %u)\n", line, n, nd, trues); ++bad; }
}
int main() {
  const char* a[] = {"Héllo", "thesé", nullptr, "ARE THE", "tést strings", "", "1.75", "-34", "+9.8", "17¼", "x³", "2³", " 12⅝",
                     "1234567890", "de", "\t\r\n\f "};
  NVStrings* s = NVStrings::create_from_array(a, 16);
  { const bool e[] = {T, T, F, F, F, F, F, F, F, T, T, T, F, T, T, F}; pred(s, &NVStrings::isalnum, e, __LINE__); }
  { const bool e[] = {T, T, F, F, F, F, F, F, F, F, F, F, F, F, T, F}; pred(s, &NVStrings::isalpha, e, __LINE__); }
  { const bool e[] = {F, F, F, F, F, F, F, F, F, F, F, F, F, F, F, T}; pred(s, &NVStrings::isspace, e, __LINE__); }
  { const bool e[] = {F, F, F, F, F, F, F, F, F, F, F, T, F, T, F, F}; pred(s, &NVStrings::isdigit, e, __LINE__); }
  { const bool e[] = {F, F, F, F, F, F, F, F, F, F, F, F, F, T, F, F}; pred(s, &NVStrings::isdecimal, e, __LINE__); }
  { const bool e[] = {F, F, F, F, F, F, F, F, F, T, F, T, F, T, F, F}; pred(s, &NVStrings::isnumeric, e, __LINE__); }
  { const bool e[] = {F, F, T, F, F, T, F, F, F, F, F, F, F, F, F, F}; pred(s, &NVStrings::is_empty, e, __LINE__); }
  { const bool e[] = {F, F, F, T, F, F, T, T, T, T, F, T, T, T, F, T}; pred(s, &NVStrings::isupper, e, __LINE__); }
  { const bool e[] = {F, T, F, F, T, F, T, T, T, T, T, T, T, T, T, T}; pred(s, &NVStrings::islower, e, __LINE__); }
  NVStrings::destroy(s);
  const char* c[] = {"Examples aBc", "thesé", nullptr, "ARE THE", "tést strings", ""};
  s = NVStrings::create_from_array(c, 6);
  { const char* e[] = {"eXAMPLES AbC", "THESÉ", nullptr, "are the", "TÉST STRINGS", ""}; CHECK(same(s->swapcase(), e, 6)); }
  { const char* e[] = {"Examples abc", "Thesé", nullptr, "Are the", "Tést strings", ""}; CHECK(same(s->capitalize(), e, 6)); }
  { const char* e[] = {"Examples Abc", "Thesé", nullptr, "Are The", "Tést Strings", ""}; CHECK(same(s->title(), e, 6)); }
  NVStrings::destroy(s);
  s = NVStrings::create_from_array(c, 0);
  bool b[1];
  CHECK(s->isalnum(b, false) == 0 && s->is_empty(b, false) == 0);
  NVStrings* t = s->title();
  CHECK(t->size() == 0);
  NVStrings::destroy(t);
  NVStrings::destroy(s);
  if (bad) return 1;
  printf("chartype host-API known answers passed\n");
  return 0;
}
"""


def test_known_answers_cpp_program():
    lib = os.path.join(ROOT, "custrings_amd")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "chartype_kat.cpp"), os.path.join(d, "chartype_kat")
        open(src, "w").write(CPP)
        subprocess.run(["g++", "-std=c++14", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                        src, "-o", exe, "-L", lib, "-lNVStrings", "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                        "-Wl,-rpath,/opt/rocm/lib"], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "known answers passed" in out.stdout


# ---- differential: generated columns against the harness ---------------------------------------------------------------------
ROWS = 1 << 20
KINDS = ["ascii", "keep", "wide", "bytes", "long", "huge"]
CASE_KINDS = KINDS + ["bytes_keep"]  # (the case ops only: arbitrary bytes on which the tile kernel's answer is the one returned)


class _CachedHarness(m.Harness):
    """(both routes of an op are held against the same harness answer: computed once)"""

    def __init__(self, *a):
        super().__init__(*a)
        self.memo = {}

    def answer(self, op, kind, arrow):
        if (op, kind) not in self.memo:
            self.memo[(op, kind)] = self.run_arrow(op, *arrow)
        return self.memo[(op, kind)]


@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield _CachedHarness(d, ROOT)


def _arbitrary_bytes(n, seed):
    """rows of arbitrary bytes: stray and missing continuation bytes, truncated characters, over-long lead bytes"""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(bytes(range(0x20, 0x7F)) * 3 + bytes(range(0x80, 0x100)) + b"\xc3\xa9\xc3\x89\xe1\xb8\x80\xf0\x9f\x98\x80\x00\t", dtype=np.uint8)
    lens = rng.integers(0, 24, size=n)
    data = alphabet[rng.integers(0, alphabet.size, size=int(lens.sum()))].tobytes()
    rows, k = [], 0
    for i, ln in enumerate(lens.tolist()):
        rows.append(None if i % 37 == 5 else data[k:k + ln])
        k += ln
    return rows


def _size_keeping(rows, harness):
    """the rows of `rows` that swapcase, capitalize and title all leave at their size, by the harness's tile mode (-2: the
    row's size would change)"""
    arrow = m.to_arrow(rows)
    keep = np.ones(len(rows), dtype=bool)
    for op in m.CASE_OPS:
        keep &= harness.run_arrow(op, *arrow, mode="tile")[0] != -2
    return [r for r, k in zip(rows, keep.tolist()) if k]


def _is_utf8(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@pytest.fixture(scope="module")
def generated(harness):
    wide = set(m.width_changing())
    ascii_pool = m.gen_rows(20_000, seed=31, kind="ascii") + m.gen_rows(10_000, seed=32, kind="uniform")
    ascii_pool = [r for r in ascii_pool if r is None or all(ord(ch) < 128 for ch in r)]
    keep_pool = [r for r in m.gen_rows(20_000, seed=33, kind="keep") if r is not None and any(ord(ch) >= 128 for ch in r)]
    wide_pool = [r for r in m.gen_rows(20_000, seed=34, kind="wide") if r is not None and any(ord(ch) in wide for ch in r)]
    # (a) and (b) draw only from characters outside the width-changing code points: their route assertions mean something
    assert not any(ord(ch) in wide for r in ascii_pool + keep_pool if r for ch in r)
    cols = {
        "ascii": m.big_column(ascii_pool, ROWS, 41),
        "keep": m.big_column(keep_pool, ROWS, 42, one_in=10, base_rows=ascii_pool),
        "wide": m.big_column(wide_pool, ROWS, 43, one_in=100, base_rows=ascii_pool),
        "bytes": _arbitrary_bytes(ROWS, 44),
    }
    long_rows = m.big_column(ascii_pool, 50_000, 45)
    for i in range(7, len(long_rows), 9973):  # a few rows beyond the staging sizes among short ones
        long_rows[i] = (b"one 100 KB row o'neil 1st " * 4000)[:100_000] if i == 7 else b"Ab c" * 2500
    long_rows[20_000] = "é1 ".encode() * 3000
    cols["long"] = long_rows
    cols["huge"] = [(b"xY z9 " * 2000) if i % 3 else ("Ünï " * 1500).encode() for i in range(600)]  # no tile fits
    # arbitrary bytes that keep their size in all three case ops: no row raises `changed`, the tile kernel's rows are the answer
    cols["bytes_keep"] = _size_keeping(_arbitrary_bytes(60_000, 46), harness)
    assert sum(r is not None and not _is_utf8(r) for r in cols["bytes_keep"]) >= 1000
    return {k: (m.to_arrow(v), column(v)) for k, v in cols.items()}


@pytest.mark.parametrize("rowwise", [False, True], ids=["tile", "rows"])
@pytest.mark.parametrize("op", m.PREDS)
def test_predicates_against_harness(generated, harness, monkeypatch, op, rowwise):
    import torch

    if rowwise:
        monkeypatch.setenv("CS_CONVERT_ROWWISE", "1")
    L = _L()
    for kind in KINDS:
        (chars, offs, nulls), g = generated[kind]
        want = harness.answer(op, kind, (chars, offs, nulls))
        rows = len(offs) - 1
        f0 = L.lib.cs_fallback_count()
        host = np.full(rows, 9, dtype=np.uint8)
        cnt = C.c_int64(-5)
        L.check(L.lib.cs_chartype(g.m_cptr, m.PREDS.index(op), host.ctypes.data, 0, None, C.byref(cnt)))
        route = _route()
        if op == "is_empty" or rowwise or kind == "huge":
            assert route == "rows", (kind, route)
        elif kind in ("ascii", "keep", "wide", "bytes"):
            assert route == "tile", (kind, route)
        assert L.lib.cs_fallback_count() == f0
        bad = np.flatnonzero(host != want)
        assert bad.size == 0, (kind, int(bad[0]), chars[offs[bad[0]]:offs[bad[0] + 1]].tobytes(), int(host[bad[0]]))
        assert cnt.value == int(want.sum())  # the return value is the number of true rows
        dev = torch.full((rows,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        cnt2 = C.c_int64(-5)
        L.check(L.lib.cs_chartype(g.m_cptr, m.PREDS.index(op), dev.data_ptr(), 1, None, C.byref(cnt2)))
        assert cnt2.value == cnt.value and np.array_equal(dev.cpu().numpy(), host), kind
        cnt3 = C.c_int64(-5)
        L.check(L.lib.cs_chartype(g.m_cptr, m.PREDS.index(op), None, 1, None, C.byref(cnt3)))  # results = 0: returns 0
        assert cnt3.value == 0


@pytest.mark.parametrize("rowwise", [False, True], ids=["tile", "rows"])
@pytest.mark.parametrize("op", m.CASE_OPS)
def test_case_ops_against_harness(generated, harness, monkeypatch, op, rowwise):
    if rowwise:
        monkeypatch.setenv("CS_CASE_ROWWISE", "1")
    L = _L()
    for kind in CASE_KINDS:
        (chars, offs, nulls), g = generated[kind]
        lens, hchars = harness.answer(op, kind, (chars, offs, nulls))
        rows = len(offs) - 1
        before = g.digest()
        f0 = L.lib.cs_fallback_count()
        out = getattr(g, op)()
        route = _route()
        if rowwise:
            assert route == "rows", kind
        elif kind in ("ascii", "keep", "long", "bytes_keep"):
            assert route == "tile", (kind, route)  # the fast route, nothing handed over
        elif kind == "wide":
            assert route == "rows", (kind, route)  # some row changes its width: the two-pass kernels recompute the column
        assert L.lib.cs_fallback_count() == f0
        assert g.digest() == before  # the input is untouched
        gchars, goffs, gvalid = out._export64()
        assert np.array_equal(np.unpackbits(gvalid, bitorder="little")[:rows].astype(bool), lens != -1), kind
        want_offs = np.zeros(rows + 1, dtype=np.int64)
        np.cumsum(np.maximum(lens, 0), out=want_offs[1:])
        assert np.array_equal(goffs, want_offs), kind
        if not np.array_equal(gchars, hchars):
            bad = int(np.argmax(gchars[: hchars.size] != hchars[: gchars.size])) if gchars.size and hchars.size else 0
            r = int(np.searchsorted(want_offs, bad, side="right") - 1)
            raise AssertionError((kind, r, chars[offs[r]:offs[r + 1]].tobytes()[:80], gchars[want_offs[r]:want_offs[r + 1]].tobytes()[:80]))
        if route == "tile":  # the output shares the input's extents
            assert np.array_equal(goffs, offs)


def test_routes_agree_on_arbitrary_bytes(generated, monkeypatch):
    """(d): the tile and the row routes give the same flags and the same columns on arbitrary bytes"""
    L = _L()
    _, g = generated["bytes"]
    rows = g.size()

    def everything():
        res = []
        for k, op in enumerate(m.PREDS):
            host = np.zeros(rows, dtype=np.uint8)
            cnt = C.c_int64()
            L.check(L.lib.cs_chartype(g.m_cptr, k, host.ctypes.data, 0, None, C.byref(cnt)))
            res.append((hashlib.sha256(host.tobytes()).hexdigest(), cnt.value))
        return res + [getattr(g, op)().digest() for op in m.CASE_OPS]

    fast = everything()
    monkeypatch.setenv("CS_CONVERT_ROWWISE", "1")
    monkeypatch.setenv("CS_CASE_ROWWISE", "1")
    assert everything() == fast


def test_empty_and_all_null_columns():
    from custrings_amd import nvstrings

    e = nvstrings.to_device([])
    n = nvstrings.to_device([None, None, None])
    for op in m.CASE_OPS:
        assert getattr(e, op)().size() == 0
        assert getattr(n, op)().to_host() == [None, None, None]
    for op in m.PREDS:
        assert getattr(e, op)() == []
        assert getattr(n, op)() == [None, None, None]
    L = _L()
    host = np.full(3, 9, dtype=np.uint8)
    cnt = C.c_int64(-1)
    L.check(L.lib.cs_is_empty(n.m_cptr, host.ctypes.data, 0, None, C.byref(cnt)))
    assert cnt.value == 3 and host.tolist() == [1, 1, 1]
    L.check(L.lib.cs_isalnum(e.m_cptr, host.ctypes.data, 0, None, C.byref(cnt)))
    assert cnt.value == 0 and host.tolist() == [1, 1, 1]  # a column of no rows: 0, nothing touched
    s = nvstrings.to_device(["o'neil mc-donald 1st", "ßx", "ḁḀ", "aⅠb"])
    assert s.title().to_host() == ["O'Neil Mc-Donald 1St", "Sx", "Ḁḁ", "AⅠB"]
    assert s.capitalize().to_host() == ["O'neil mc-donald 1st", "Sx", "ḁḀ", "AⅠb"]
    assert s.swapcase().to_host() == ["O'NEIL MC-DONALD 1ST", "SX", "Ḁḁ", "AⅰB"]


def test_gpu_full_size_chartype_routes_agree():
    """isalnum and title on the FULL 100M-row C3 column, tile route against row route, by a digest of the flags / of the column"""
    import torch

    L = _L()
    g = gpuutil.synth(3, 0, 100_000_000)
    rows = g.size()
    flags = torch.empty(rows, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def run():
        cnt = C.c_int64()
        L.check(L.lib.cs_isalnum(g.m_cptr, flags.data_ptr(), 1, None, C.byref(cnt)))
        r1 = _route()
        # a digest of the flags: their count and a position-weighted sum (int64 arithmetic on the device, exact)
        w = torch.arange(rows, dtype=torch.int64, device="cuda") % 1000003
        d = (int(flags.sum(dtype=torch.int64)), int((flags.to(torch.int64) * w).sum()))
        assert d[0] == cnt.value
        t = g.title()
        return r1, d, _route(), t.digest()

    f0 = L.lib.cs_fallback_count()
    fast = run()
    assert fast[0] == "tile" and fast[2] == "tile" and L.lib.cs_fallback_count() == f0
    for name in ("CS_CONVERT_ROWWISE", "CS_CASE_ROWWISE"):
        L.check(L.lib.cs_config_set(name.encode(), b"1"))
    try:
        slow = run()
    finally:
        for name in ("CS_CONVERT_ROWWISE", "CS_CASE_ROWWISE"):
            L.check(L.lib.cs_config_set(name.encode(), None))
    assert slow[0] == "rows" and slow[2] == "rows"
    assert fast[1] == slow[1] and fast[3] == slow[3]
