"""The substring / padding / wrapping ops on the MI355X: the reference's known answers through the Python API, the pyni
glue and a C++ program built against include/nvstrings; 1M-row columns against the CPU harness of pad_ops.h (checked
against the model by tests/test_pad_cpu.py) for every op on both routes, with accents, nulls, rows beyond the staging
sizes; wrap's shared extents; the argument errors; an output of more than 2 GiB checked by windows."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cpulibs
import gpuutil
import pad_model as m

pytestmark = pytest.mark.gpu

ROOT = cpulibs.ROOT


def cases():
    with open(os.path.join(ROOT, "tests", "golden", "reference_pad.json")) as f:
        return json.load(f)["cases"]


def _lib():
    return gpuutil.lib()


def _route():
    return _lib().lib.cs_debug_last_route().decode()


def column(rows):
    from custrings_amd import nvstrings

    chars, offs, nulls = m.to_arrow(rows)
    valid = np.packbits(1 - nulls, bitorder="little")
    valid = np.concatenate([valid, np.zeros(8, dtype=np.uint8)])
    return nvstrings.from_offsets64(chars if chars.size else np.zeros(1, dtype=np.uint8), offs, len(rows), valid)


def exported(g):
    chars, offs, valid = g._export64()
    bits = np.unpackbits(valid, bitorder="little")[: g.size()]
    data, o = chars.tobytes(), offs.tolist()
    return [data[o[i]:o[i + 1]] if bits[i] else None for i in range(g.size())]


def _call(s, case):
    """the golden case through the nvstrings API"""
    args, kw = case["args"], case["kwargs"]
    if case["op"] == "slice_from":
        a = list(args) + [None, None]
        return s.slice_from(starts=kw.get("starts", a[0]) or 0, stops=kw.get("stops", a[1]) or 0)
    if case["api"] == "cpp":  # (the member's order -> the Python API's)
        args = m.member_args(case["op"], args, "cpp")
        if case["op"] == "slice_replace":
            args = [args[1], args[2], args[0]]
        elif case["op"] == "insert":
            args = [args[1], args[0]]
    return getattr(s, case["op"])(*args, **kw)


@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s-%s" % (c["op"], c["src"].split(":")[-1], c["args"]))
def test_known_answers_python_api(case):
    from custrings_amd import nvstrings

    s = nvstrings.to_device(case["input"])
    assert _call(s, case).to_host() == case["expected"], case["src"]


@pytest.mark.parametrize("case", cases(), ids=lambda c: "%s-%s-%s" % (c["op"], c["src"].split(":")[-1], c["args"]))
def test_known_answers_pyni_glue(case):
    import torch

    import pyniNVStrings as P

    h = P.n_createFromHostStrings(case["input"])
    try:
        args = m.member_args(case["op"], case["args"], case["api"])
        op = case["op"]
        keep = []
        if op == "slice_from":
            a = list(case["args"]) + [None, None]
            ptrs = []
            for v in (case["kwargs"].get("starts", a[0]), case["kwargs"].get("stops", a[1])):
                if v is None:
                    ptrs.append(0)
                else:
                    t = torch.tensor(v, dtype=torch.int32, device="cuda")
                    keep.append(t)
                    ptrs.append(t.data_ptr())
            torch.cuda.synchronize()
            r = P.n_slice_from(h, *ptrs)
        elif op == "slice_replace":
            r = P.n_slice_replace(h, args[1], args[2], args[0])
        elif op == "insert":
            r = P.n_insert(h, args[1], args[0])
        elif op == "pad":
            r = P.n_pad(h, args[0], args[1] if len(args) > 1 else "left", args[2] if len(args) > 2 else " ")
        elif op in ("ljust", "rjust", "center"):
            r = getattr(P, "n_" + op)(h, args[0], args[1] if len(args) > 1 else None)
        else:
            r = getattr(P, "n_" + op)(h, *args)
        try:
            assert P.n_createHostStrings(r) == case["expected"], case["src"]
        finally:
            P.n_destroyStrings(r)
    finally:
        P.n_destroyStrings(h)


CPP = r"""
#include <cstdio>
#include <cstring>
#include <stdexcept>
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
int main() {
  const char* p[] = {"12345", "thesé", nullptr, "ARE THE", "tést strings", ""};
  NVStrings* s = NVStrings::create_from_array(p, 6);
  { const char* e[] = {"1234512345", "theséthesé", nullptr, "ARE THEARE THE", "tést stringstést strings", ""}; CHECK(same(s->repeat(2), e, 6)); }
  { const char* e[] = {"12345     ", "thesé     ", nullptr, "ARE THE   ", "tést strings", "          "}; CHECK(same(s->ljust(10), e, 6)); }
  { const char* e[] = {"  12345", "  thesé", nullptr, "ARE THE", "tést strings", "       "}; CHECK(same(s->rjust(7), e, 6)); }
  { const char* e[] = {"__12345__", "__thesé__", nullptr, "_ARE THE_", "tést strings", "_________"}; CHECK(same(s->center(9, "_"), e, 6)); }
  { const char* e[] = {"__12345__", "__thesé__", nullptr, "_ARE THE_", "tést strings", "_________"}; CHECK(same(s->pad(9, NVStrings::both, "_"), e, 6)); }
  { const char* e[] = {"00012345", "000thesé", nullptr, "0ARE THE", "tést strings", "00000000"}; CHECK(same(s->zfill(8), e, 6)); }
  { const char* e[] = {"12345", "thesé", nullptr, "ARE\nTHE", "tést\nstrings", ""}; CHECK(same(s->wrap(3), e, 6)); }
  NVStrings::destroy(s);
  const char* q[] = {"Héllo", "thesé", nullptr, "ARE THE", "tést strings", ""};
  s = NVStrings::create_from_array(q, 6);
  { const char* e[] = {"Hé___lo", "th___sé", nullptr, "AR___ THE", "té___t strings", "___"}; CHECK(same(s->slice_replace("___", 2, 3), e, 6)); }
  { const char* e[] = {"Héllox", "theséx", nullptr, "ARE THEx", "tést stringsx", "x"}; CHECK(same(s->slice_replace("x", -1, -1), e, 6)); }
  { const char* e[] = {"l", "e", nullptr, "E", "s", ""}; CHECK(same(s->slice(2, 3), e, 6)); }
  { const char* e[] = {"lo", "sé", nullptr, " THE", "t strings", ""}; CHECK(same(s->slice(3, -1), e, 6)); }
  { const char* e[] = {"H", "t", nullptr, "A", "t", ""}; CHECK(same(s->get(0), e, 6)); }
  { const char* e[] = {"H***éllo", "t***hesé", nullptr, "A***RE THE", "t***ést strings", ""}; CHECK(same(s->insert("***", 1), e, 6)); }
  { const char* e[] = {"Héllo++", "thesé++", nullptr, "ARE THE++", "tést strings++", "++"}; CHECK(same(s->insert("++", -1), e, 6)); }
  {
    int h[6] = {4, 4, 4, 4, 4, 4};
    int* d = nullptr;
    CHECK(hipMalloc(&d, sizeof(h)) == hipSuccess);
    CHECK(hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) == hipSuccess);
    const char* e[] = {"o", "é", nullptr, "THE", " strings", ""};
    CHECK(same(s->slice_from(d), e, 6));
    CHECK(hipFree(d) == hipSuccess);
  }
  bool threw = false;
  try { s->slice(5, 2); } catch (const std::invalid_argument&) { threw = true; }
  CHECK(threw);
  threw = false;
  try { s->slice_replace(nullptr, 1, 2); } catch (const std::invalid_argument&) { threw = true; }
  CHECK(threw);
  threw = false;
  try { s->insert(nullptr, 1); } catch (const std::invalid_argument&) { threw = true; }
  CHECK(threw);
  threw = false;
  try { s->repeat(0xFFFFFFFFu); } catch (const std::invalid_argument&) { threw = true; }
  CHECK(threw);
  NVStrings::destroy(s);
  if (bad) return 1;
  printf("pad host-API known answers passed\n");
  return 0;
}
"""


def test_known_answers_cpp_program():
    lib = os.path.join(ROOT, "custrings_amd")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "pad_kat.cpp"), os.path.join(d, "pad_kat")
        open(src, "w").write(CPP)
        subprocess.run(["g++", "-std=c++14", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                        src, "-o", exe, "-L", lib, "-lNVStrings", "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                        "-Wl,-rpath,/opt/rocm/lib"], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "known answers passed" in out.stdout


# ---- differential: generated columns against the harness ---------------------------------------------------------------------
ROWS = 1 << 20
SETTINGS = [
    ("slice", dict(start=2, stop=12), lambda g: g.slice(2, 12)),
    ("slice", dict(start=0, stop=1), lambda g: g.get(0)),
    ("slice", dict(start=-1, stop=5), lambda g: g.slice(-1, 5)),
    ("slice", dict(start=1, stop=20, step=3), lambda g: g.slice(1, 20, 3)),
    ("slice_replace", dict(repl="_é_".encode(), start=2, stop=5), lambda g: g.slice_replace(2, 5, "_é_")),
    ("slice_replace", dict(repl=b"x", start=-1, stop=-1), lambda g: g.slice_replace(-1, -1, "x")),
    ("insert", dict(repl=b"**", start=3), lambda g: g.insert(3, "**")),
    ("insert", dict(repl=b"+", start=-1), lambda g: g.insert(-1, "+")),
    ("repeat", dict(reps=3), lambda g: g.repeat(3)),
    ("ljust", dict(width=30), lambda g: g.ljust(30)),
    ("rjust", dict(width=24, fill="é".encode()), lambda g: g.rjust(24, "é")),
    ("center", dict(width=21, fill=b"_"), lambda g: g.center(21, "_")),
    ("zfill", dict(width=20), lambda g: g.zfill(20)),
    ("wrap", dict(width=6), lambda g: g.wrap(6)),
]


@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


@pytest.fixture(scope="module")
def generated():
    short = m.gen_rows(ROWS, seed=21)
    mixed = m.gen_rows(50_000, seed=22)
    for i in range(0, len(mixed), 997):  # rows over 6 KB among short ones: tiles beyond the staging sizes
        mixed[i] = (mixed[i] or b"") + "é".encode() * 3500
    return {"short": (short, column(short)), "mixed": (mixed, column(mixed))}


@pytest.mark.parametrize("rowwise", [False, True], ids=["tile", "rows"])
@pytest.mark.parametrize("k", range(len(SETTINGS)), ids=lambda k: "%s-%d" % (SETTINGS[k][0], k))
def test_against_harness(generated, harness, monkeypatch, k, rowwise):
    if rowwise:
        monkeypatch.setenv("CS_PAD_ROWWISE", "1")
    op, kw, call = SETTINGS[k]
    for which, (rows, g) in generated.items():
        chars, offs, nulls = m.to_arrow(rows)
        lens, hchars = harness.run_arrow(op, chars, offs, nulls, **kw)
        out = call(g)
        assert _route() == ("rows" if rowwise else "tile"), which
        gchars, goffs, gvalid = out._export64()
        assert np.array_equal(np.unpackbits(gvalid, bitorder="little")[: len(rows)].astype(bool), lens != -1), which
        want_offs = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum(np.maximum(lens, 0), out=want_offs[1:])
        assert np.array_equal(goffs, want_offs), which
        if not np.array_equal(gchars, hchars):
            bad = int(np.argmax(gchars[: hchars.size] != hchars[: gchars.size])) if gchars.size and hchars.size else 0
            r = int(np.searchsorted(want_offs, bad, side="right") - 1)
            raise AssertionError((which, r, rows[r], exported(out.sublist(r, r + 1))))
        if op == "wrap":  # the output shares the input's extents
            _, ioffs, _ = g._export64()
            assert np.array_equal(goffs, ioffs)


# ---- a staged tile whose output exceeds the out-tile ----------------------------------------------------------------------------
# the host's tile plan, restated (cs_plan.hip plan_row_tiles / plan_staged_tiles, sized_route.h write_sized)
PF_BYTES, STAGE_SLACK, OUT_TILE, WAVE_ROW = 6144, 48, 16 * 1024, 256


def tile_plan(rows, out_rows):
    """-> per tile (first row, end row, its input is staged wherever the chars begin, its output bytes).  The plan takes the
    largest R of 64 / 32 / 16 whose widest R-row span + 32 fits the prefetch, else 64-row tiles sized for all but a few; a
    tile's input is staged when its span, up to 15 bytes of lead and the slack fit the wave's buffer; pad then assembles
    the tile in the LDS out-tile unless its output exceeds OUT_TILE (such a tile goes from memory to memory)."""
    def offsets(rr):
        return np.concatenate([[0], np.cumsum([0 if x is None else len(x) for x in rr])])

    offs, oo, n = offsets(rows), offsets(out_rows), len(rows)
    R, span = 64, PF_BYTES - 64
    for cand in (64, 32, 16):
        widest = max(int(offs[min(r0 + cand, n)] - offs[r0]) for r0 in range(0, n, cand))
        if widest + 32 <= PF_BYTES:
            R, span = cand, widest
            break
    cap = (span + STAGE_SLACK + 15) & ~15
    return [(r0, min(r0 + R, n), int(offs[min(r0 + R, n)] - offs[r0]) + 15 + STAGE_SLACK <= cap, int(oo[min(r0 + R, n)] - oo[r0]))
            for r0 in range(0, n, R)]


LONG_ROW = 129  # in the last tile (rows 128 .. 133), beside a null row and an empty one
GROW_SETTINGS = {
    # op: (harness arguments, the model's, the call, the long row's tile leaves through the LDS out-tile)
    "repeat": (dict(reps=4), [4], lambda g: g.repeat(4), False),  # 22 KB: from memory, the long row by the whole wave
    "ljust": (dict(width=300), [300], lambda g: g.ljust(300), True),  # (the 64-row tiles do not fit: rows of 300 bytes by the wave)
    "slice": (dict(start=1, stop=20, step=3), [1, 20, 3], lambda g: g.slice(1, 20, 3), True),  # strided: never by the wave
    "slice_replace": (dict(repl="_é_".encode(), start=2, stop=5), ["_é_", 2, 5], lambda g: g.slice_replace(2, 5, "_é_"), True),
    "wrap": (dict(width=6), [6], lambda g: g.wrap(6), True),
}


@pytest.fixture(scope="module")
def grow(harness):
    """-> (rows, device column, {op: the harness's rows, which are the model's})"""
    rows = m.gen_rows(134, seed=31, maxlen=6)
    rows[40] = "abc dé ".encode() * 700  # 5600 bytes: its tile is the column's widest, so that the tile under test is staged
    rows[128:] = [b"ab", "ab é€ 中-😀\t7 ".encode() * 275, None, b"", "é x".encode(), b"-7\tz"]  # (whatever its first byte's address)
    assert len(rows) == 134 and len(rows[LONG_ROW]) == 5500
    want = {}
    for op, (kw, args, _, through_lds) in GROW_SETTINGS.items():
        want[op] = harness.run(op, rows, **kw)
        assert want[op] == m.apply_column(op, rows, args), op
        plan = tile_plan(rows, want[op])
        r0, r1, staged, out_span = plan[-1]
        assert (r0, r1) == (128, 134) and staged and (out_span <= OUT_TILE) == through_lds, (op, plan[-1])
        if op == "ljust":  # the full tiles spill, and every row of theirs goes by the wave
            assert all(o > OUT_TILE for _, _, _, o in plan[:-1]) and all(r is None or len(r) > WAVE_ROW for r in want[op][:128])
    return rows, column(rows), want


@pytest.mark.parametrize("rowwise", [False, True], ids=["tile", "rows"])
@pytest.mark.parametrize("op", list(GROW_SETTINGS))
def test_staged_tile_with_output_beyond_the_out_tile(grow, monkeypatch, op, rowwise):
    if rowwise:
        monkeypatch.setenv("CS_PAD_ROWWISE", "1")
    rows, g, want = grow
    out = GROW_SETTINGS[op][2](g)
    assert _route() == ("rows" if rowwise else "tile")
    gchars, goffs, gvalid = out._export64()
    assert np.array_equal(np.unpackbits(gvalid, bitorder="little")[: len(rows)].astype(bool), [r is not None for r in rows])
    assert goffs.tolist() == np.concatenate([[0], np.cumsum([0 if r is None else len(r) for r in want[op]])]).tolist()
    assert gchars.tobytes() == b"".join(r for r in want[op] if r is not None)


def test_slice_from_against_harness(generated, harness, monkeypatch):
    import torch

    rows, g = generated["short"]
    rng = np.random.default_rng(8)
    st = rng.integers(-3, 30, size=len(rows)).astype(np.int32)
    sp = rng.integers(-3, 30, size=len(rows)).astype(np.int32)
    chars, offs, nulls = m.to_arrow(rows)
    for rowwise in (False, True):
        if rowwise:
            monkeypatch.setenv("CS_PAD_ROWWISE", "1")
        for s, e in ((st, sp), (st, None), (None, sp)):
            lens, hchars = harness.run_arrow("slice", chars, offs, nulls, starts=s, stops=e)
            for host in (True, False):
                a = s if host or s is None else torch.from_numpy(s).cuda()
                b = e if host or e is None else torch.from_numpy(e).cuda()
                out = g.slice_from(starts=0 if a is None else a, stops=0 if b is None else b)
                gchars, goffs, _ = out._export64()
                assert np.array_equal(gchars, hchars), (rowwise, host)
                assert _route() == ("rows" if rowwise else "tile")


def test_argument_errors():
    from custrings_amd import nvstrings

    L = _lib()
    s = nvstrings.to_device(["abc", None, "déf"])
    out = C.c_void_p()
    assert L.lib.cs_slice(s.m_cptr, 5, 2, 1, None, C.byref(out)) == L.CS_ERR_INVALID_ARG
    assert L.lib.cs_slice_replace(s.m_cptr, None, 1, 2, None, C.byref(out)) == L.CS_ERR_INVALID_ARG
    assert L.lib.cs_insert(s.m_cptr, None, 1, None, C.byref(out)) == L.CS_ERR_INVALID_ARG
    assert L.lib.cs_repeat(s.m_cptr, 0xFFFFFFFF, None, C.byref(out)) == L.CS_ERR_RANGE
    assert L.lib.cs_pad(s.m_cptr, 0x80000000, 1, None, None, C.byref(out)) == L.CS_ERR_RANGE
    assert L.lib.cs_pad(s.m_cptr, 5, 3, None, None, C.byref(out)) == L.CS_ERR_INVALID_ARG
    with pytest.raises(Exception):
        s.slice(5, 2)
    with pytest.raises(Exception):
        s.slice_replace(1, 2, None)
    with pytest.raises(ValueError):
        s.ljust(5, "")
    assert s.slice(5, 0).to_host() == ["", None, ""]  # stop 0 is the end
    assert nvstrings.to_device(["accénted"]).slice(2, 8, 2).to_host() == ["cne"]  # deviation 1: no NUL byte
    assert s.repeat(0).to_host() == ["abc", None, "déf"]
    e = nvstrings.to_device([])
    assert e.ljust(4).size() == 0 and e.wrap(3).size() == 0


def test_output_over_2gib_checked_by_windows(harness):
    import torch

    from custrings_amd import nvstrings

    L = _lib()
    n = 95_000_000
    gen = torch.Generator(device="cuda").manual_seed(6)
    lens = torch.randint(0, 16, (n,), dtype=torch.int64, device="cuda", generator=gen)
    offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens, 0, out=offs[1:])
    total = int(offs[-1])
    chars = torch.randint(0x61, 0x7B, (total + 64,), dtype=torch.uint8, device="cuda", generator=gen)
    torch.cuda.synchronize()
    g = nvstrings.from_offsets64(chars, offs, n, bdevmem=True)
    del chars
    out = g.ljust(24)
    assert _route() == "tile"
    assert int(L.lib.cs_column_nbytes(out.m_cptr)) == 24 * n  # >= 2^31
    h_offs = offs.cpu().numpy()
    for w0 in (0, n // 3, n - 40_000):
        w1 = w0 + 40_000
        rows = exported(g.sublist(w0, w1))
        assert exported(out.sublist(w0, w1)) == harness.run("ljust", rows, width=24)
        assert int(h_offs[w1] - h_offs[w0]) == sum(len(r) for r in rows)
    _, ooffs, _ = out.sublist(n - 3, n)._export64()
    assert ooffs.tolist() == [0, 24, 48, 72]
