"""from_csv on the GPU, bit for bit against the model (tests/csv_model.py) through the C ABI: the fixture file and the
reference's known answers, the flags against sort, host bytes against device bytes, `lines`, and the places where the
two-level line scan carries state -- sizes around a scan tile, control-byte runs across tile boundaries and longer than two
tiles, NUL bytes at a boundary --, the row-wise route of the field walk, and the output's metadata."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import cpulibs
import csv_model as m
import gpuutil

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(cpulibs.ROOT, "tests", "golden")
HEAD = os.path.join(GOLDEN, "tweets_head.csv")


def host(g):
    return gpuutil.to_col(g).to_bytes_list() if g.size() else []


def last_route():
    return gpuutil.lib().lib.cs_debug_last_route().decode()


def load(data, column=0, lines=0, flags=0, device=False, skew=0):
    """cs_column_from_csv_buffer over host bytes, or over a device copy of them `skew` bytes off a 16-byte boundary"""
    from custrings_amd import nvstrings

    L = gpuutil.lib()
    out = C.c_void_p()
    if device:
        import torch

        t = torch.frombuffer(bytearray(b"\xee" * skew + bytes(data) + b"\xee"), dtype=torch.uint8).cuda()[skew:skew + len(data)]
        L.check(L.lib.cs_column_from_csv_buffer(t.data_ptr(), len(data), 1, column, lines, flags, None, C.byref(out)))
        torch.cuda.synchronize()
    else:
        arr = np.frombuffer(bytes(data) + b"\xee", dtype=np.uint8)
        L.check(L.lib.cs_column_from_csv_buffer(arr.ctypes.data, len(data), 0, column, lines, flags, None, C.byref(out)))
    return nvstrings.nvstrings(out.value)


def check(data, column=0, lines=0, flags=0, where=("host", "device")):
    want = m.from_csv_buffer(data, column, lines, flags)
    for w in where:
        got = load(data, column, lines, flags, device=w != "host", skew=3 if w == "skewed" else 0)
        assert host(got) == want, (w, column, lines, flags, len(data))
    return want


@functools.lru_cache(maxsize=None)
def tile():
    return int(gpuutil.lib().lib.cs_csv_tile_bytes())


@functools.lru_cache(maxsize=None)
def mixed(nbytes):
    """`nbytes` bytes of well-formed mixed lines (the last one cut)"""
    text = m.gen_lines(nbytes // 20 + 8, seed=9, shape="mixed")
    assert len(text) >= nbytes
    return text[:nbytes]


# ---- the fixture file and the known answers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("column", [0, 6, 7, 8])
def test_fixture_file_columns(column):
    from custrings_amd import nvstrings

    L = gpuutil.lib()
    out = C.c_void_p()
    L.check(L.lib.cs_column_from_csv(HEAD.encode(), column, 0, 0, None, C.byref(out)))
    got = nvstrings.nvstrings(out.value)
    assert host(got) == m.from_csv(HEAD, column) and got.size() == 63


def test_known_answers_through_python_from_csv(tmp_path):
    import nvstrings as top

    with open(os.path.join(GOLDEN, "reference_csv.json")) as f:
        tweets, doc = json.load(f)["cases"]
    got = top.from_csv(HEAD, tweets["column"])
    assert got.to_host()[:tweets["first"]] == tweets["expected"]
    p = tmp_path / "file.csv"
    p.write_text(doc["text"])
    assert top.from_csv(str(p), doc["column"]).to_host() == doc["expected"]
    assert top.from_csv_buffer(doc["text"].encode(), doc["column"]).to_host() == doc["expected"]


def test_python_from_csv_buffer_takes_arrays_and_tensors():
    import torch

    import nvstrings as top

    data = mixed(1000)
    want = m.from_csv_buffer(data, 1)
    assert host(top.from_csv_buffer(np.frombuffer(data, dtype=np.uint8), 1)) == want
    assert host(top.from_csv_buffer(torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(), 1)) == want


def test_refused_files_give_none(tmp_path):
    import nvstrings as top

    assert top.from_csv(str(tmp_path / "missing.csv"), 0) is None
    for data in (b"", b"x"):
        p = tmp_path / "tiny.csv"
        p.write_bytes(data)
        assert top.from_csv(str(p), 0) is None
    assert host(load(b"abc\0\nd\n")) == [] and host(load(b"")) == []  # (no line end in front of the first NUL: an empty column)


# ---- flags and lines --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [1, 2, 3, 8, 9, 10])
def test_flags_against_sort_of_the_unsorted_column(flags):
    from custrings_amd import nvstrings

    L = gpuutil.lib()
    data = mixed(6000)
    for column in (1, 7):
        check(data, column, 0, flags, where=("host",))
        got = load(data, column, 0, flags)
        plain = load(data, column, 0, flags & 8)
        if flags & 3:
            out = C.c_void_p()
            L.check(L.lib.cs_sort(plain.m_cptr, flags & 3, 1, 1, None, C.byref(out)))
            plain = nvstrings.nvstrings(out.value)
        assert host(got) == host(plain)
    nulls = sum(r is None for r in m.from_csv_buffer(data, 1))
    assert nulls >= 5 and m.from_csv_buffer(data, 1, 0, 8).count(b"") >= nulls


def test_lines_limits():
    data = mixed(3000)
    rows = len(m.from_csv_buffer(data, 0))
    for lines in (1, 2, rows - 1, rows, rows + 1, rows + 1000):
        assert len(check(data, 2, lines)) == min(rows, lines)


def test_host_bytes_against_device_bytes():
    data = mixed(20000)
    for column in (0, 4, 7, 30):
        check(data, column, where=("host", "device", "skewed"))
    check(data + b"\n", 30, where=("host", "device", "skewed"))  # (the last row runs into the appended '\r', which device bytes do not hold)
    check(b"h\na,b", 1, where=("host", "device", "skewed"))


# ---- the scan's carries -----------------------------------------------------------------------------------------------------------
def at_tile(spec):
    """'3T+5' -> 3 * tile() + 5"""
    mult, has_tile, add = spec.partition("T")
    return int(mult or 1) * tile() + int(add or 0) if has_tile else int(spec)


@pytest.mark.parametrize("size", ["T-1", "T", "T+1", "3T+5", "T-2", "16", "17"])
def test_sizes_around_a_tile(size):
    n = at_tile(size)
    for data in (mixed(n), mixed(n - 1) + b"\n", b"h" + b"\n" * (n - 1)):
        assert len(data) == n
        check(data, 1)


def lead(n):
    """n bytes: a header, a few lines, the last byte no control byte"""
    body = b"h0,h1\n" + b"ab,cd\n" * ((n - 7) // 6)
    return body + b"x" * (n - len(body))


@pytest.mark.parametrize("run", [b"\t\n\t\t", b"\t\t\n\t", b"\t\t\t\t", b"\n\t\t\t", b"\t\t\t\n"])
@pytest.mark.parametrize("tiles", [1, 2])
def test_a_control_run_across_a_tile_boundary(run, tiles):
    T = tile()
    data = lead(tiles * T - 2) + run + b"b,c\nd,e\n"
    assert data[tiles * T - 2:tiles * T + 2] == run
    want = check(data, 0)
    assert (b"b" in want) == (b"\n" in run)  # (without a terminator the run is part of a line: "b" begins no row of its own)


@pytest.mark.parametrize("terminator", [None, 0, "middle", "last"])
def test_a_control_run_longer_than_two_tiles(terminator):
    T = tile()
    run = bytearray(b"\t\x01" * (T + 9))
    if terminator is not None:
        run[{0: 0, "middle": T + 3, "last": len(run) - 1}[terminator]] = 0x0D
    data = lead(T // 2 + 5) + bytes(run) + b"b,c\nd,e\n"
    want = check(data, 0)
    assert (b"b" in want) == (terminator is not None)


def test_a_tile_that_is_one_line_without_a_terminator():
    T = tile()
    data = lead(T - 40) + b"\n" + b"y," * (T + 30) + b"\nq,r\n"
    want = check(data, 1)
    assert want[-2:] == [b"y", b"r"] and last_route() == "rows"


def test_a_quote_pair_split_by_a_tile_boundary():
    T = tile()
    head = lead(T - 11) + b'\n"abcdefgh'
    assert len(head) == T - 1
    data = head + b'""x",z\nq,r\n'
    assert data[T - 1:T + 1] == b'""'
    want = check(data, 0)
    assert want[-2:] == [b'abcdefgh""x', b"q"]


@pytest.mark.parametrize("at", ["T-1", "T", "T+1", "2T+40", "3T+4", "0", "1"])
def test_the_first_nul(at):
    T = tile()
    data = bytearray(mixed(3 * T + 5))
    p = at_tile(at)
    data[p] = 0
    data[3 * T + 2] = 0  # (a later NUL changes nothing)
    want = check(bytes(data), 1)
    assert len(want) < len(m.from_csv_buffer(mixed(3 * T + 5), 1))
    data[p - 1] = 0x0A  # a line start AT the NUL: the row before it is whole
    check(bytes(data), 1)


def test_one_row_beyond_the_staged_tile_goes_row_wise():
    data = b"h0,h1\n" + b"ab,cd\n" * 200 + b"k," + b'"' + b"w, " * 4000 + b'",z\n' + b"ab,cd\n" * 200
    want = check(data, 1, where=("host",))
    assert last_route() == "rows" and max(len(r) for r in want) == 12000
    check(b"h0,h1\n" + b"ab,cd\n" * 400, 1, where=("host",))
    assert last_route() == "tile"


def test_ten_thousand_generated_lines():
    data = m.gen_lines(10000, seed=10, shape="mixed")
    for column in (0, 7):
        assert len(check(data, column)) == 10000  # (\n\n is one line end: a blank line is no row)
    noisy = b"".join(m.gen_buffers(4000, seed=11, nul_rate=0.0))
    for column in (0, 2):
        check(noisy, column, where=("host", "skewed"))


def test_the_output_hands_on_its_metadata():
    got = load(mixed(30000), 7)
    span, longest = gpuutil.cached_meta(got)[:2]
    assert (span, longest) == gpuutil.measured_meta(got) and longest > 0
