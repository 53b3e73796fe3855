"""The cases of tests/test_gpu_radix.py reach the edges of the radix sort they claim to (no GPU needed): every digit
position, every pass count, a skipped digit that is not zero, long runs of one digit inside a wave's chunk -- and the numpy
reference the GPU test compares with agrees with Python's own stable sort.  `pytest -s` prints the coverage table."""
import numpy as np
import pytest

import radix_cases as rc


@pytest.fixture(scope="module")
def cases():
    """(name, n, keys, live digit positions) of every case the GPU test runs."""
    out = []
    for name in rc.FAMILIES:
        for n in rc.sizes(name):
            keys = rc.keys_of(name, n)
            out.append((name, n, keys, rc.live_digit_positions(keys)))
    return out


def test_every_family_runs_at_every_small_size_and_the_marked_ones_beyond(cases):
    have = {(name, n) for name, n, _, _ in cases}
    for name, (_, large) in rc.FAMILIES.items():
        for n in rc.SMALL_N:
            assert (name, n) in have
        for n in rc.LARGE_N:
            assert ((name, n) in have) == large
    assert ("full_random", rc.HUGE_N) in have
    assert 3 * rc.TILE + 1 in rc.LARGE_N and rc.HUGE_N >= 300_000
    assert (max(rc.LARGE_N) + rc.TILE - 1) // rc.TILE * 256 > 4096, "the (digit, tile) counts of the largest (L) size fit one scan block"
    for want in ("full_random", "two_keys_99_to_1", "already_sorted", "strictly_reverse_sorted"):
        assert rc.FAMILIES[want][1]


def test_each_digit_position_is_live_and_each_pass_count_occurs(cases):
    by_digit = {d: [] for d in range(8)}
    by_passes = {p: [] for p in range(9)}
    for name, n, keys, live in cases:
        for d in live:
            by_digit[d].append((name, n))
        by_passes[len(live)].append((name, n))
    for d in range(8):
        print("digit %d live in %d cases, alone in %s" % (d, len(by_digit[d]), sorted({nm for nm, n, k, lv in cases if lv == [d]})))
        assert by_digit[d], "no case with a live digit %d" % d
        assert any(lv == [d] for _, _, _, lv in cases), "no case whose only pass is digit %d" % d
    for p in range(9):
        print("%d passes: %d cases, e.g. %s" % (p, len(by_passes[p]), by_passes[p][-1:]))
        assert by_passes[p], "no case with %d passes" % p
    # an odd pass count leaves the result in the scratch buffers (the copy back), an even one in the caller's
    assert any(len(lv) % 2 == 1 and n > rc.TILE for _, n, _, lv in cases) and any(len(lv) % 2 == 0 and lv and n > rc.TILE for _, n, _, lv in cases)


def test_the_families_give_the_pass_counts_they_are_named_for():
    n = 4097
    assert rc.live_digit_positions(rc.keys_of("full_random", n)) == list(range(8))
    for d in range(8):
        assert rc.live_digit_positions(rc.keys_of("live_digit_%d_of_256_values" % d, n)) == [d]
        assert rc.live_digit_positions(rc.keys_of("live_digit_%d_of_2_values" % d, n)) == [d]
        assert len(np.unique(rc.digit(rc.keys_of("live_digit_%d_of_2_values" % d, n), d))) == 2
    for k, live in rc.LIVE_SETS.items():
        assert rc.live_digit_positions(rc.keys_of("%d_live_digits" % k, n)) == list(live)
    assert {2, 3, 5, 7} <= set(rc.LIVE_SETS)
    for name in ("all_equal_zero", "all_equal_ones", "all_equal_mixed"):
        assert rc.live_digit_positions(rc.keys_of(name, n)) == []
    firsts = [int(rc.keys_of(nm, 2)[0]) for nm in ("all_equal_zero", "all_equal_ones", "all_equal_mixed")]
    assert firsts[:2] == [0, rc.ONES] and firsts[2] not in (0, rc.ONES)
    for where, at in (("first", 0), ("last", n - 1), ("middle", n // 2)):
        for d, nm in ((7, "top"), (0, "bottom")):
            keys = rc.keys_of("one_differs_%s_in_the_%s_digit" % (where, nm), n)
            assert rc.live_digit_positions(keys) == [d]
            assert np.flatnonzero(keys != keys[(at + 1) % n]).tolist() == [at]
    two = rc.keys_of("two_keys_99_to_1", 70_001)
    vals, counts = np.unique(two, return_counts=True)
    assert len(vals) == 2 and 0.005 < counts.min() / len(two) < 0.02
    s = rc.keys_of("already_sorted", n)
    assert (s[1:] >= s[:-1]).all()
    r = rc.keys_of("strictly_reverse_sorted", rc.LARGE_N[-1])
    assert (r[1:] < r[:-1]).all()
    e = rc.keys_of("extremes", n)
    assert {0, 1, (1 << 63) - 1, 1 << 63, rc.ONES} <= set(int(x) for x in e)
    low = e & np.uint64((1 << 63) - 1)
    assert any(len(set(int(x) for x in e[low == v])) == 2 for v in np.unique(low)), "no two keys that differ in bit 63 only"
    # the callers' shapes: many duplicates each
    for name in ("order_keys", "order_keys_descending", "order_keys_with_nulls", "tie_keys"):
        keys = rc.keys_of(name, 8193)
        assert len(np.unique(keys)) < len(keys) * 0.8, name
    o = rc.keys_of("order_keys", 8193)
    assert int((o & np.uint64(0xFFFFFFFF)).max()) < 3000 and int((o >> np.uint64(32)).max()) == 301
    c = ~rc.keys_of("order_keys_descending", 8193)  # (its own draw, complemented)
    assert int((c & np.uint64(0xFFFFFFFF)).max()) < 3000 and int((c >> np.uint64(32)).max()) == 301
    w = rc.keys_of("order_keys_with_nulls", 8193)
    assert 0.01 < (w == 0).mean() < 0.04 and 0.01 < (w == np.uint64(rc.ONES)).mean() < 0.04
    t = rc.keys_of("tie_keys", 8193)
    assert set(np.unique(t & np.uint64(0xFF)).tolist()) == set(range(16))


def test_some_skipped_digit_is_not_zero(cases):
    found = []
    for name, n, keys, live in cases:
        if n > 1 and live:
            skipped = [d for d in range(8) if d not in live and rc.digit(keys, d)[0] != 0]
            below = [d for d in skipped if d < max(live)]  # ... and between passes that run, not only above the last one
            if below and min(live) < min(below):
                found.append((name, n, below))
    print("non-zero skipped digits between live ones: %d cases, e.g. %s" % (len(found), found[:2]))
    assert found
    # ... and a case with nothing but non-zero skipped digits: zero passes over keys that are not zero
    assert any(n > 1 and not live and keys[0] != 0 for _, n, keys, live in cases)


def test_long_runs_of_one_digit_inside_a_waves_chunk(cases):
    """The running count per digit in LDS: a wave ranks its 1024 pairs in 16 steps of 64, so a digit value held by more than
    64 pairs of an aligned 1024-pair chunk is counted across steps.  A chunk cannot hold more than 1024 pairs: the most there
    is to ask is a chunk whose pairs ALL hold one value in a pass that runs (1024 equal digits -- thousands per tile), beside
    chunks where a value has more than 64 but not all, and tiles where one value has more than 1024 pairs (the waves' totals
    become each wave's start)."""
    part, whole, across = [], [], []
    for name, n, keys, live in cases:
        if not live:
            continue
        d = min(live)  # the first pass that runs sees the input order
        c, size = rc.most_equal_digits(keys, d, rc.CHUNK)
        if 64 < c < size:
            part.append((name, n, c))
        if c == size == rc.CHUNK:
            whole.append((name, n, c))
        t, _ = rc.most_equal_digits(keys, d, rc.TILE)
        if t > rc.CHUNK:
            across.append((name, n, t))
    print("one digit value on more than 64 pairs of a chunk, not all: %d cases, most %s" % (len(part), max(part, key=lambda x: x[2])))
    print("one digit value on all 1024 pairs of a chunk in a pass that runs: %d cases, e.g. %s" % (len(whole), whole[:2]))
    print("one digit value on more than 1024 pairs of a tile: %d cases, most %s" % (len(across), max(across, key=lambda x: x[2])))
    assert part and whole and across
    assert any(c > 512 for _, _, c in part), "no chunk split about evenly between two values (the 2-value live digits)"
    assert any(t >= rc.TILE - 1 for _, _, t in across), "no tile with (all but) one bucket empty"


def test_the_numpy_reference_is_pythons_stable_sort():
    n = 1000
    for name in rc.FAMILIES:
        keys, items = rc.keys_of(name, n), rc.items_of(name, n)
        want = sorted(range(n), key=lambda i: int(keys[i]))
        got_keys, got_items = rc.reference(keys, items)
        assert got_keys.tolist() == [int(keys[i]) for i in want], name
        assert got_items.tolist() == [int(items[i]) for i in want], name
    items = rc.items_of("full_random", 4097)
    assert items.dtype == np.int32 and (items < 0).any() and (items > 0).any() and not np.array_equal(items, np.arange(4097))
