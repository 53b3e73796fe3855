"""url_encode / url_decode / translate / fillna / index / rindex on the GPU, bit for bit against the model
(tests/recode_model.py): the three sized ops on both routes (tile, and rows through CS_RECODE_ROWWISE) at the row counts and
row lengths where each mechanism can go wrong, the reference's known answers, the decode and translate quirks, fillna's
nulls, index / rindex's errors, the output's metadata in front of a tile op, borrowed inputs at an odd address, and the
Python methods and the n_* glue once each."""
import contextlib
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import borrowedutil as bu
import cpulibs
import gpuutil
import pad_model
import recode_model as m

pytestmark = pytest.mark.gpu

SIZED = ["url_encode", "url_decode", "translate"]
ROUTES = ["tile", "rows"]
EURO, GRIN = 0x20AC, 0x1F600
# widths both ways, a 4-byte key, a delete; ' ' -> a 3-byte character grows the long row of the "grow" shape 3x
TABLE = [[ord(" "), EURO], [0xE9, ord("e")], [EURO, GRIN], [GRIN, 0xDF], [0x4E2D, 0], [ord("b"), 0xF1], [0, ord("0")]]


def cases():
    with open(os.path.join(cpulibs.ROOT, "tests", "golden", "reference_recode.json")) as f:
        return json.load(f)["cases"]


def dev(rows):
    """bytes / None rows -> device column (the binary-safe ingest)"""
    from custrings_amd import nvstrings

    if not rows:
        return nvstrings.to_device([])
    chars, offs, valid = bu.arrow(rows)
    return nvstrings.from_offsets64(chars if chars.size else np.zeros(1, dtype=np.uint8), offs, len(rows), valid)


def host(g):
    return gpuutil.to_col(g).to_bytes_list() if g.size() else []


def null_count(g):
    return int(gpuutil.lib().lib.cs_column_null_count(g.m_cptr))


def call(fn, *args):
    """a producing C entry point -> (status, column or None)"""
    from custrings_amd import nvstrings

    L = gpuutil.lib()
    out = C.c_void_p()
    st = getattr(L.lib, fn)(*args, None, C.byref(out))
    return st, (nvstrings.nvstrings(out.value) if out.value else None)


def sized(op, g, pairs=None):
    L = gpuutil.lib()
    if op == "translate":
        pairs = pairs or []
        k = np.array([p[0] for p in pairs], dtype=np.uint32)
        v = np.array([p[1] for p in pairs], dtype=np.uint32)
        st, out = call("cs_translate", g.m_cptr, k.ctypes.data if pairs else None, v.ctypes.data if pairs else None, len(pairs))
    else:
        st, out = call("cs_" + op, g.m_cptr)
    L.check(st)
    return out


@contextlib.contextmanager
def routed(route):
    L = gpuutil.lib()
    L.check(L.lib.cs_config_set(b"CS_RECODE_ROWWISE", b"1" if route == "rows" else None))
    try:
        yield
    finally:
        L.check(L.lib.cs_config_set(b"CS_RECODE_ROWWISE", None))


def last_route():
    return gpuutil.lib().lib.cs_debug_last_route().decode()


def check_sized(op, rows, g, route, pairs=None, want=None):
    want = m.apply_column(op, rows, pairs) if want is None else want
    with routed(route):
        out = sized(op, g, pairs)
        if rows:
            assert last_route() == route
    assert host(out) == want
    assert null_count(out) == sum(r is None for r in rows)
    return out


# ---- the host's tile plan, restated (cs_plan.hip plan_row_tiles / plan_staged_tiles, cs_recode.hip run_recode) ---------------------
PF_BYTES, STAGE_SLACK, OUT_TILE = 6144, 48, 16 * 1024


def tile_plan(rows, out_rows, r):
    """-> (row r's tile is staged in LDS wherever the chars begin, the output bytes of that tile).  The plan takes the
    largest R of 64 / 32 / 16 whose widest R-row span + 32 fits the prefetch, else 64-row tiles sized for all but a few; a
    tile is staged when its span, up to 15 bytes of lead and the slack fit the wave's buffer; it leaves through the LDS
    out-tile unless its output exceeds OUT_TILE."""
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
    r0 = r // R * R
    r1 = min(r0 + R, n)
    return int(offs[r1] - offs[r0]) + 15 + STAGE_SLACK <= cap, int(oo[r1] - oo[r0])


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape(name):
    """-> (rows, device column, {op: the model's rows})"""
    body = m.gen_rows(1100, seed=21)
    if name == "0":
        rows = []
    elif name == "1":
        rows = [b"a b%41\xc3\xa9%"]
    elif name == "65":
        rows = body[:65]
    elif name == "1100":
        rows = body
    elif name == "all-null":
        rows = [None] * 200
    elif name == "no-bytes":
        rows = [b""] * 130
    elif name == "row-7000":  # beyond the input stage
        rows = list(body)
        rows[517] = (b"ab %41\xe2\x82\xac-%" * 700)[:7000]
    elif name == "grow":
        # the long row's tile is STAGED (its input fits the wave's buffer) and its output exceeds the 16 KB out-tile: the lanes
        # write to memory out of LDS.  A longer row of unreserved bytes in another tile makes that one the column's widest, so
        # that the tile under test fits whatever its first byte's address is (tile_plan checks it)
        rows = list(body)
        rows[333] = b" " * 5500
        rows[700] = b"a" * 5600
    else:  # "grow-both": the input exceeds the stage as well (read from memory, written to memory)
        rows = list(body)
        rows[333] = b" " * 6000
    want = {op: m.apply_column(op, rows, TABLE) for op in SIZED}
    if name in ("grow", "grow-both"):
        for op in ("url_encode", "translate"):
            staged, out_span = tile_plan(rows, want[op], 333)
            assert staged == (name == "grow") and out_span > OUT_TILE, (name, op, staged, out_span)
    if name == "row-7000":
        assert not tile_plan(rows, want["url_decode"], 517)[0]
    return rows, dev(rows), want


SHAPES = ["0", "1", "65", "1100", "all-null", "no-bytes", "row-7000", "grow", "grow-both"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("op", SIZED)
@pytest.mark.parametrize("name", SHAPES)
def test_sized_ops_match_the_model(name, op, route):
    rows, g, want = shape(name)
    out = check_sized(op, rows, g, route, TABLE, want[op])
    assert out.size() == len(rows)


# ---- the reference's known answers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", [c for c in cases() if c["op"] in SIZED], ids=lambda c: "%s-%s-%s" % (c["op"], c["src"].split("/")[-1], c.get("table", "")))
def test_known_answers_sized(case, route):
    rows = [None if r is None else r.encode() for r in case["input"]]
    assert m.apply_case(case) == case["expected"]
    check_sized(case["op"], rows, dev(rows), route, case["args"], [None if e is None else e.encode() for e in case["expected"]])


@pytest.mark.parametrize("case", [c for c in cases() if c["op"] not in SIZED], ids=lambda c: "%s-%s" % (c["op"], c["src"].split("/")[-1]))
def test_known_answers_fillna_and_index(case):
    from custrings_amd import nvstrings

    g = nvstrings.to_device(case["input"])
    if case["op"] == "fillna":
        a = case["args"]
        got = g.fillna(a["str"] if "str" in a else nvstrings.to_device(a["column"]))
        assert got.to_host() == case["expected"] == m.apply_case(case)
    else:
        assert getattr(g, case["op"])(*case["args"]) == case["expected"] == m.apply_case(case)


# ---- decode -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_decode_stops_at_the_row_boundary_and_keeps_its_quirks(route):
    # "%4" ends a row and "1" starts the next: nothing is decoded across them -- inside a tile (rows 0 / 1) and where one
    # 64-row tile ends and the next begins (rows 63 / 64)
    rows = [b"a%4", b"1b"] + [b"r%d%%2%d" % (i, i % 10) for i in range(61)] + [b"x%4", b"1y", b"%", b"4", b"1"]
    rows += m.percent_tail_rows() + [b"%%41", b"%%%", b"%e2%82%ac", b"%zz", b"%4", b"a%", b"%41"]
    assert rows[63] == b"x%4" and rows[64] == b"1y"
    want = m.apply_column("url_decode", rows)
    assert want[0] == b"a%4" and want[1] == b"1b" and want[63] == b"x%4" and want[64] == b"1y"
    assert want[-7:] == [b"\x041", b"\x00", "€".encode(), b"\x53", b"%4", b"a%", b"A"]
    check_sized("url_decode", rows, dev(rows), route, None, want)


# ---- translate ---------------------------------------------------------------------------------------------------------------------
ASCII_TABLE = [[ord("a"), ord("A")], [ord("%"), 0], [ord(" "), ord("_")], [0, ord("0")]]
TRANSLATE_CASES = {
    "empty-table": ("mixed", []),
    "ascii-table-ascii-rows": ("ascii", ASCII_TABLE),
    "ascii-table-mixed-rows": ("mixed", ASCII_TABLE),
    "4-byte-key": ("mixed", [[GRIN, ord("!")], [ord("Z"), GRIN]]),
    "delete-everything": ("mixed", [[ord(c), 0] for c in sorted(set("".join(m.ALPHABET)))]),
    "300-keys": ("mixed", [[0x100 + k, EURO if k % 3 == 0 else ord("a") + k % 26] for k in range(300)] + [[0xE9, GRIN], [0x4E2D, 0], [0xE9, 0xF1]]),
}


@functools.lru_cache(maxsize=None)
def translate_rows(kind):
    rows = [r for r in m.gen_rows(1100, seed=22) if r is not None]
    if kind == "ascii":
        rows = [bytes(c for c in r if c < 0x80) for r in rows]
    return rows, dev(rows)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(TRANSLATE_CASES))
def test_translate_tables(name, route):
    kind, pairs = TRANSLATE_CASES[name]
    rows, g = translate_rows(kind)
    out = check_sized("translate", rows, g, route, pairs)
    if name == "empty-table":
        assert host(out) == rows
    if name == "delete-everything":
        assert host(out) == [b""] * len(rows) and null_count(out) == 0
    if name == "300-keys":  # (the duplicate key 0xE9: the last pair wins -- every é became ñ, none of them a 4-byte character)
        src, dst = b"".join(rows), b"".join(host(out))
        n_e = src.count("é".encode())
        assert n_e > 0 and dst.count("ñ".encode()) == src.count("ñ".encode()) + n_e and dst.count("😀".encode()) == src.count("😀".encode())


def test_translate_refuses_a_code_point_beyond_unicode():
    _, g, _ = shape("65")
    k, v = np.array([ord("a"), 0x110000], dtype=np.uint32), np.array([ord("b"), ord("c")], dtype=np.uint32)
    assert call("cs_translate", g.m_cptr, k.ctypes.data, v.ctypes.data, 2)[0] == 1  # CS_ERR_INVALID_ARG
    assert call("cs_translate", g.m_cptr, v.ctypes.data, k.ctypes.data, 2)[0] == 1
    assert call("cs_translate", g.m_cptr, None, None, 2)[0] == 1


# ---- fillna ---------------------------------------------------------------------------------------------------------------------------
def test_fillna():
    rows = m.gen_rows(1100, seed=23, null_rate=0.3)
    g = dev(rows)
    assert null_count(g) > 100
    for repl in (b"", "é€😀".encode(), b"||"):
        st, out = call("cs_fillna", g.m_cptr, repl)
        assert st == 0 and host(out) == m.fillna_column(rows, repl) and null_count(out) == 0
    # a column with nulls at the same rows (every third null of `rows`) and at other rows
    other = m.gen_rows(1100, seed=24, null_rate=0.3)
    k = 0
    for i, r in enumerate(rows):
        if r is None:
            k += 1
            if k % 3 == 0:
                other[i] = None
    want = m.fillna_column(rows, other)
    both = sum(r is None for r in want)
    assert 0 < both < sum(r is None for r in rows)
    go = dev(other)  # (held: a column lives as long as its Python object)
    st, out = call("cs_fillna_column", g.m_cptr, go.m_cptr)
    assert st == 0 and host(out) == want and null_count(out) == both
    # nothing to fill, everything to fill, no rows
    full = [r or b"" for r in rows]
    gf = dev(full)
    st, out = call("cs_fillna_column", gf.m_cptr, go.m_cptr)
    assert st == 0 and host(out) == full and null_count(out) == 0
    gn, g0 = dev([None] * 70), dev([])
    st, out = call("cs_fillna", gn.m_cptr, b"xy")
    assert st == 0 and host(out) == [b"xy"] * 70
    st, out = call("cs_fillna", g0.m_cptr, b"xy")
    assert st == 0 and out.size() == 0


def test_fillna_argument_errors():
    _, g, _ = shape("65")
    _, h, _ = shape("1100")
    assert call("cs_fillna_column", g.m_cptr, h.m_cptr) == (1, None)  # CS_ERR_INVALID_ARG: another row count
    assert call("cs_fillna", g.m_cptr, None) == (1, None)
    assert call("cs_fillna_column", g.m_cptr, None) == (1, None)
    with pytest.raises(ValueError):
        g.fillna(h)
    with pytest.raises(ValueError):
        g.fillna(None)


# ---- index / rindex ---------------------------------------------------------------------------------------------------------------------
def test_index_and_rindex():
    import torch
    from custrings_amd import nvstrings

    rows = ["he-llo", "-there-", None, "accént-éd", "-"]
    g = nvstrings.to_device(rows)
    assert g.index("-") == [2, 0, None, 6, 0] and g.rindex("-") == [2, 6, None, 6, 0]
    miss = nvstrings.to_device(["a-b", "ab", None, "-", "b"])
    for fn in (miss.index, miss.rindex):
        with pytest.raises(ValueError, match="not found in element 1"):
            fn("-")
    # the device form: the results are in the caller's buffer either way; null rows count as found
    buf = torch.full((5,), 77, dtype=torch.int32, device="cuda")
    assert g.index("-", devptr=buf.data_ptr()) == buf.data_ptr()
    torch.cuda.synchronize()
    assert buf.cpu().tolist() == [2, 0, -2, 6, 0]
    assert g.rindex("-", devptr=buf.data_ptr()) == buf.data_ptr()
    assert buf.cpu().tolist() == [2, 6, -2, 6, 0]
    buf.fill_(77)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="not found in 2 elements"):
        miss.index("-", devptr=buf.data_ptr())
    assert buf.cpu().tolist() == [1, -1, -2, 0, -1]
    with pytest.raises(ValueError, match="not found in 2 elements"):
        miss.rindex("-", devptr=buf.data_ptr())


# ---- the output's metadata -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("op", SIZED)
def test_metadata_from_the_scan_serves_a_tile_op(op, route):
    """the scan's longest row and largest 64-row span go to the output: slice (a tile op) plans its tiles from them"""
    rows = [None if i % 11 == 5 else ("ab c%%41é-%d € x" % i).encode() for i in range(2049)]
    pairs = [[ord("c"), EURO], [0xE9, ord("e")]]
    with routed(route):
        out = sized(op, dev(rows), pairs)
    mid = m.apply_column(op, rows, pairs)
    got = out.slice(1, 6)
    assert last_route() == "tile"
    assert got.to_host() == [None if r is None else pad_model.apply("slice", r.decode(), [1, 6]) for r in mid]


# ---- borrowed input ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", SIZED)
def test_borrowed_column_at_an_odd_address(op):
    rows = m.gen_rows(300, seed=25)
    rows[0], rows[-1] = b"%41 first", b"last %4"
    # (ASCII poison: the byte behind the chars is '1' -- "last %4" must not become "last A" -- and the one in front '7')
    src = bu.Borrowed(rows, 7, 8, bu.poison_for("ascii", "num"))
    want = m.apply_column(op, rows, TABLE)
    for route in ROUTES:
        with routed(route):
            out = sized(op, src.col, TABLE)
        assert host(out) == want, route
    assert src.caller_memory_intact()


# ---- the Python methods and the n_* glue --------------------------------------------------------------------------------------------------------
def test_python_methods():
    from custrings_amd import nvstrings

    s = ["a b/é", None, "100%", "%41%zz", ""]
    g = nvstrings.to_device(s)
    dec = lambda rows: [None if r is None else r.decode("utf-8", "surrogateescape") for r in rows]
    b = [None if r is None else r.encode() for r in s]
    assert g.url_encode().to_host() == dec(m.apply_column("url_encode", b))
    assert g.url_decode().to_host() == dec(m.apply_column("url_decode", b))
    assert g.translate(str.maketrans("a%", "A#", "/")).to_host() == [None if r is None else r.translate(str.maketrans("a%", "A#", "/")) for r in s]
    assert g.translate([["é", "e"], ["b", None], [" ", "€"]]).to_host() == ["a€/e", None, "100%", "%41%zz", ""]
    assert g.translate({}).to_host() == s and g.translate([]).to_host() == s
    for bad in ("ab", None, 5, [["a"]], [["a", "b", "c"]], ["ab"]):
        with pytest.raises(ValueError):
            g.translate(bad)
    assert g.fillna("é").to_host() == ["é" if r is None else r for r in s]
    assert g.fillna(nvstrings.to_device(["1", "2", "3", None, "5"])).to_host() == ["a b/é", "2", "100%", "%41%zz", ""]


def test_pyni_glue():
    import torch

    import pyniNVStrings as P

    s = ["a b/é", None, "100%", "%41-", "-"]
    h = P.n_createFromHostStrings(s)
    made = []

    def rows(r):
        made.append(r)
        return P.n_createHostStrings(r)

    try:
        assert rows(P.n_url_encode(h)) == ["a%20b%2F%C3%A9", None, "100%25", "%2541-", "-"]
        assert rows(P.n_url_decode(h)) == ["a b/é", None, "100%", "A-", "-"]
        assert rows(P.n_translate(h, {ord("a"): ord("A"), ord("/"): None, 0xE9: 0x20AC})) == ["A b€", None, "100%", "%41-", "-"]
        assert rows(P.n_translate(h, [["b", "B"], ["%", None]])) == ["a B/é", None, "100", "41-", "-"]
        for bad in ("ab", 7, None, [["a"]], [["a", "b", "c"]]):
            with pytest.raises(ValueError):
                P.n_translate(h, bad)
        assert rows(P.n_fillna(h, "é")) == ["a b/é", "é", "100%", "%41-", "-"]
        o = P.n_createFromHostStrings(["1", "2", "3", "4", "5"])
        made.append(o)
        with pytest.raises(ValueError):
            P.n_fillna(h, None)
        short = P.n_createFromHostStrings(["1"])
        made.append(short)

        class Holder:  # (an object written for the reference's glue carries the pointer in m_cptr)
            def __init__(self, p):
                self.m_cptr = p

        assert rows(P.n_fillna(h, Holder(o))) == ["a b/é", "2", "100%", "%41-", "-"]
        with pytest.raises(ValueError):
            P.n_fillna(h, Holder(short))
        d = P.n_createFromHostStrings(["a-b", None, "--"])
        made.append(d)
        assert P.n_index(d, "-", 0, None, 0) == [1, None, 0] and P.n_rindex(d, "-", 0, None, 0) == [1, None, 1]
        with pytest.raises(ValueError, match="not found in element 0"):
            P.n_index(d, "b", 1, 2, 0)
        buf = torch.full((3,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert P.n_rindex(d, "-", 0, None, buf.data_ptr()) == buf.data_ptr()
        assert buf.cpu().tolist() == [1, -2, 1]
        with pytest.raises(ValueError, match="not found in 1 elements"):
            P.n_index(d, "b", 0, None, buf.data_ptr())
        assert buf.cpu().tolist() == [2, -2, -1]
    finally:
        for r in made:
            P.n_destroyStrings(r)
        P.n_destroyStrings(h)
