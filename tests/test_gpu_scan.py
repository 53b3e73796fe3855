"""The lengths-to-offsets scan under every output column (cs::Built::scan), by itself, against numpy.

cs_debug_offsets_from_lengths runs one of the library's five scan routes over a device array of int32 lengths; nothing here
allocates chars, so a row may be gigabytes long.  Offsets, column total, validity mask and the two sizing numbers a later tile
kernel trusts (longest row, largest 64-row span) are compared for EXACT equality with

    offsets  = [0] + cumsum(maximum(lens, 0))            (int64)
    validity = packbits(lens >= 0, little) padded with zero bytes to validity_bytes(n)
    max_row  = max(maximum(lens, 0));  max_span64 = largest sum over rows [64k, min(64k + 64, n))

Routes: 0 chunk scan, 1 chunk scan fused with validity, 2 workgroup scan (CS_SCAN_BY_WORKGROUPS), 3 the scan that reads
nothing back, 4 the segmented scan."""
import numpy as np
import pytest

import gpuutil

pytestmark = pytest.mark.gpu

ROUTES = (0, 1, 2, 3, 4)
GUARD = 8  # int64 sentinels behind the offsets: a store past segs * (n + 1) shows
SENTINEL = -0x0123456789ABCDEF


def reference(lens):
    """(offsets, validity bytes, max_row, max_span64) of one segment."""
    lens = np.asarray(lens, dtype=np.int32)
    n = len(lens)
    clipped = np.maximum(lens, 0).astype(np.int64)
    offsets = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(clipped, dtype=np.int64)])
    validity = np.zeros((n + 63) // 64 * 8, dtype=np.uint8)
    bits = np.packbits(lens >= 0, bitorder="little")
    validity[: len(bits)] = bits
    starts = np.arange(0, n, 64)
    ends = np.minimum(starts + 64, n)
    return offsets, validity, int(clipped.max()), int((offsets[ends] - offsets[starts]).max())


def run(lens_dev, n, route, segs=1):
    """Runs `route` over the device tensor lens_dev (segs * n int32).  -> (offsets [segs, n + 1], validity or None, out [segs, 3])"""
    import torch

    L = gpuutil.lib()
    assert lens_dev.dtype == torch.int32 and lens_dev.numel() == segs * n
    offs = torch.full((segs * (n + 1) + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    valid = torch.full(((n + 63) // 64 * 8,), 0xFF, dtype=torch.uint8, device="cuda") if route == 1 else None
    out = np.full(3 * segs, -7, dtype=np.int64)
    torch.cuda.synchronize()
    L.check(L.lib.cs_debug_offsets_from_lengths(lens_dev.data_ptr(), n, segs, route, offs.data_ptr(), valid.data_ptr() if valid is not None else None,
                                                out.ctypes.data, None))
    got = offs.cpu().numpy()
    assert (got[segs * (n + 1):] == SENTINEL).all(), "route %d wrote behind offsets[segs * (n + 1)]" % route
    return got[: segs * (n + 1)].reshape(segs, n + 1), (valid.cpu().numpy() if valid is not None else None), out.reshape(segs, 3)


def to_dev(lens):
    import torch

    return torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).cuda()


def check(lens, route, lens_dev=None, ref=None, what=""):
    """One segment on one route against the reference, everything the route reports."""
    n = len(lens)
    what = "%s route %d n %d" % (what, route, n)
    offsets, validity, max_row, max_span = ref if ref is not None else reference(lens)
    got, gvalid, out = run(to_dev(lens) if lens_dev is None else lens_dev, n, route)
    bad = np.flatnonzero(got[0] != offsets)
    assert bad.size == 0, "%s: %d offsets differ, the first at row %d: %d, expected %d" % (what, bad.size, bad[0], got[0][bad[0]], offsets[bad[0]])
    assert out[0, 0] == offsets[n], what + ": total"
    if route == 1:
        assert np.array_equal(gvalid, validity), what + ": validity"
    if route in (0, 1, 2):
        assert (int(out[0, 1]), int(out[0, 2])) == (max_row, max_span), what + ": (max_row, max_span64)"
    elif route == 3:
        assert (out[0, 1], out[0, 2]) == (-1, -1), what
    else:
        assert (int(out[0, 1]), out[0, 2]) == (max_row, -1), what + ": largest"


EDGE_N = [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n", EDGE_N)
def test_gpu_scan_at_the_edges_of_lane_chunk_and_workgroup(n, route):
    """A lane holds 4 lengths, a wave a 2048-row chunk, a workgroup four chunks (route 2: a thread a length, a workgroup 256)."""
    rng = np.random.default_rng(1000 + n)
    check(rng.integers(-1, 40, size=n), route)


def test_gpu_scan_of_no_rows():
    import torch

    L = gpuutil.lib()
    lens = torch.zeros(4, dtype=torch.int32, device="cuda")
    for route in ROUTES:
        offs = torch.full((1 + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
        out = np.full(3, -7, dtype=np.int64)
        torch.cuda.synchronize()
        L.check(L.lib.cs_debug_offsets_from_lengths(lens.data_ptr(), 0, 1, route, offs.data_ptr(), None, out.ctypes.data, None))
        got = offs.cpu().numpy()
        assert got[0] == 0 and out[0] == 0 and (got[1:] == SENTINEL).all(), route


# ---- the second sweep of k_scan_block_sums: more than 8192 chunk (or block) sums ----------------------------------------
SWEEP_CHUNKS = 2048 * 8192
SWEEP_BLOCKS = 256 * 8192


@pytest.fixture(scope="module")
def sweep():
    """16 777 217 lengths on the device with their reference offsets, made once; a shorter case is a prefix of both."""
    rng = np.random.default_rng(8192)
    lens = rng.integers(-1, 40, size=SWEEP_CHUNKS + 1).astype(np.int32)
    for edge in (SWEEP_BLOCKS, SWEEP_CHUNKS):  # nulls on both sides of either sweep edge, whatever the generator drew
        lens[edge - 3] = -1
        if edge + 2 < len(lens):
            lens[edge + 2] = -1
    clipped = np.maximum(lens, 0).astype(np.int64)
    offsets = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(clipped, dtype=np.int64)])
    dev = to_dev(lens)
    offsets.setflags(write=False)
    lens.setflags(write=False)
    return lens, offsets, dev


def sweep_case(sweep, n, route):
    lens, offsets, dev = sweep
    starts = np.arange(0, n, 64)
    ends = np.minimum(starts + 64, n)
    validity = np.zeros((n + 63) // 64 * 8, dtype=np.uint8)
    bits = np.packbits(lens[:n] >= 0, bitorder="little")
    validity[: len(bits)] = bits
    ref = (offsets[: n + 1], validity, int(lens[:n].max()), int((offsets[ends] - offsets[starts]).max()))
    check(lens[:n], route, lens_dev=dev[:n], ref=ref, what="second sweep")


@pytest.mark.parametrize("route", (0, 1, 3))
@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_gpu_scan_carries_across_8192_chunk_sums(sweep, delta, route):
    sweep_case(sweep, SWEEP_CHUNKS + delta, route)


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_gpu_scan_carries_across_8192_block_sums(sweep, delta):
    sweep_case(sweep, SWEEP_BLOCKS + delta, 2)


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_gpu_segmented_scan_carries_across_8192_block_sums(sweep, delta):
    """(route 4 shares the sweep with route 2; its segments are `n` apart in the sums)"""
    n = SWEEP_BLOCKS + delta
    lens, offsets, dev = sweep
    got, _, out = run(dev[: 2 * n], n, 4, segs=2)
    for k in range(2):
        want = offsets[k * n: (k + 1) * n + 1] - offsets[k * n]
        assert np.array_equal(got[k], want), "segment %d" % k
        assert out[k, 0] == want[-1] and out[k, 1] == int(lens[k * n: (k + 1) * n].max())


# ---- content ------------------------------------------------------------------------------------------------------------
def content_cases():
    rng = np.random.default_rng(77)
    for n in (257, 4100):
        last_only = np.zeros(n, dtype=np.int32)
        last_only[-1] = 9
        null_last = rng.integers(0, 40, size=n).astype(np.int32)
        null_last[-1] = -1
        tenth = rng.integers(0, 60, size=n).astype(np.int32)
        tenth[rng.random(n) < 0.10] = -1
        yield "all_null_%d" % n, np.full(n, -1, dtype=np.int32)
        yield "all_empty_%d" % n, np.zeros(n, dtype=np.int32)
        yield "only_the_last_row_%d" % n, last_only
        yield "null_in_the_last_row_%d" % n, null_last
        yield "a_tenth_null_%d" % n, tenth
    for row in (63, 64, 2047, 2048):
        one = np.zeros(4100, dtype=np.int32)
        one[row] = 5000
        yield "5000_at_row_%d" % row, one
        # the same beside a smaller span on the other side of the window edge: a span credited to the wrong window shows
        two = np.zeros(4100, dtype=np.int32)
        two[row] = 5000
        two[row - 1 if row % 64 == 0 else row + 1] = 4000
        yield "5000_at_row_%d_4000_next_door" % row, two


CONTENT = list(content_cases())


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name,lens", CONTENT, ids=[c[0] for c in CONTENT])
def test_gpu_scan_content(name, lens, route):
    check(lens, route, what=name)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shift", (1, 2, 3))
def test_gpu_scan_of_lengths_at_a_dword_aligned_address(shift, route):
    """load_chunk reads 16 bytes a lane at whatever dword the lengths start: a view 4, 8 and 12 bytes into an aligned buffer."""
    import torch

    n = 2048 + 5
    rng = np.random.default_rng(shift)
    lens = rng.integers(-1, 40, size=n).astype(np.int32)
    big = torch.full((n + 16,), 1 << 30, dtype=torch.int32, device="cuda")  # (what lies around would wreck every sum)
    assert big.data_ptr() % 16 == 0
    big[shift: shift + n] = to_dev(lens)
    view = big[shift: shift + n]
    assert view.data_ptr() % 16 == 4 * shift
    check(lens, route, lens_dev=view, what="shift %d" % shift)


# ---- the switch between 32-bit and 64-bit sums -----------------------------------------------------------------------------
def wide_cases():
    rng = np.random.default_rng(31)
    n = 4096
    a = np.ones(n, dtype=np.int64)
    a[:2048] = 1 << 20  # the first chunk's total is exactly 2^31: wide; the second chunk's 2048: narrow
    yield "chunk_of_2_to_31_then_a_narrow_one", a
    b = np.full(n, 1 << 20, dtype=np.int64)
    b[5] -= 2  # 0x7ffffffe: the largest narrow total
    b[2048 + 5] -= 1  # 0x7fffffff: the smallest wide one
    yield "chunk_totals_7ffffffe_and_7fffffff", b
    b2 = b.copy()
    b2[5], b2[2048 + 5] = b[2048 + 5], b[5]
    yield "chunk_totals_7fffffff_and_7ffffffe", b2
    c = rng.integers(-1, 40, size=n).astype(np.int64)
    c[8] = c[9] = (1 << 31) - 1
    yield "two_rows_of_int_max_in_one_lane", c
    d = rng.integers(-1, 40, size=n).astype(np.int64)
    d[64:128] = 1 << 25  # one wave of the first workgroup sums to 2^31, its three neighbours stay small
    yield "one_wave_of_2_to_31", d
    for total, name in ((0x7FFFFFFE, "7ffffffe"), (0x7FFFFFFF, "7fffffff")):
        e = rng.integers(0, 40, size=n).astype(np.int64)
        e[128:192] = 0
        e[128 + 17] = total - 1000
        e[128 + 40] = 1000
        yield "one_wave_total_" + name, e
    # (a lane scans a ROUND of 256 lengths at a time: the 32-bit form goes wrong once a round, not the chunk, reaches 2^31)
    for short, name in ((0, "one_round_of_2_to_31"), (1, "one_round_total_7fffffff")):
        g = np.zeros(n, dtype=np.int64)
        g[256:512] = 1 << 23
        g[300] -= short
        g[2048:] = rng.integers(-1, 40, size=n - 2048)
        yield name, g
    f = rng.integers(-1, 40, size=n).astype(np.int64)
    f[2047], f[2048] = (1 << 31) - 1, (1 << 31) - 1  # either side of the chunk edge, one 64-row window apart
    yield "int_max_either_side_of_the_chunk_edge", f


WIDE = list(wide_cases())
assert all(lens.max() <= 0x7FFFFFFF and lens.min() >= -1 for _, lens in WIDE)
WIDE = [(name, lens.astype(np.int32)) for name, lens in WIDE]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name,lens", WIDE, ids=[c[0] for c in WIDE])
def test_gpu_scan_switches_to_64_bit_sums(name, lens, route):
    """k_chunk_offsets scans a chunk in 32 bits when its total is below 0x7fffffff, block_exclusive_scan a wave; the
    metadata is exact here too (max_span64 is an int64, max_row fits an int)."""
    check(lens, route, what=name)


# ---- the segmented scan ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segs", (1, 2, 5))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 8191, 8192, 8193))
def test_gpu_segmented_scan(n, segs):
    """Independent random segments: per-segment offsets and totals, and the largest length of each (what findall and extract
    size their columns' rows with)."""
    rng = np.random.default_rng(100 * n + segs)
    lens = rng.integers(-1, 40, size=(segs, n)).astype(np.int32)
    lens[rng.integers(0, segs), rng.integers(0, n)] = 3000  # (the largest differs from segment to segment)
    got, _, out = run(to_dev(lens.reshape(-1)), n, 4, segs=segs)
    for k in range(segs):
        offsets, _, max_row, _ = reference(lens[k])
        assert np.array_equal(got[k], offsets), "segment %d of %d, n %d" % (k, segs, n)
        assert (out[k, 0], out[k, 1]) == (offsets[n], max_row), "segment %d of %d, n %d: (total, largest)" % (k, segs, n)


def test_gpu_scan_entry_point_refuses_what_it_does_not_run():
    import torch

    L = gpuutil.lib()
    lens = torch.zeros(8, dtype=torch.int32, device="cuda")
    offs = torch.zeros(32, dtype=torch.int64, device="cuda")
    out = np.zeros(6, dtype=np.int64)
    for n, segs, route in ((4, 2, 0), (4, 1, 5), (4, 1, -1), (-1, 1, 0), (4, 0, 4)):
        assert L.lib.cs_debug_offsets_from_lengths(lens.data_ptr(), n, segs, route, offs.data_ptr(), None, out.ctypes.data, None) == L.CS_ERR_INVALID_ARG
