"""The key families and sizes of tests/test_gpu_radix.py (the stable LSD sort of cs_radix.hip by itself), kept apart from it
so that tests/test_radix_cases_cpu.py can check, without a GPU, that the cases reach the edges they are there for.

A family is a function (n, rng) -> n uint64 keys.  The sort works on eight 8-bit digits, digit d = bits [8d, 8d + 8); a pass
runs for every digit that takes more than one value among the keys.  A workgroup ranks a tile of 4096 pairs, each of its four
waves a chunk of 1024 consecutive pairs in 16 ballot steps of 64."""
import zlib

import numpy as np

TILE = 4096
CHUNK = 1024
FILL = 0xA5  # the constant byte of the digits that are not live: a skipped digit is not zero

SMALL_N = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193]
LARGE_N = [3 * TILE + 1, 70_001]  # a last tile of one pair; 18 tiles: 4608 (digit, tile) counts, more than one scan block
HUGE_N = 300_000  # (full random only)

U64 = np.uint64
ONES = 0xFFFFFFFFFFFFFFFF
FILLED = int.from_bytes(bytes([FILL] * 8), "little")


def _u64(values):
    return np.ascontiguousarray(values, dtype=U64)


def _with_digits(n, rng, live, values):
    """FILL in every byte, the digits in `live` drawn from `values` distinct byte values."""
    keys = np.full(n, FILLED, dtype=U64)
    for d in live:
        byte = rng.integers(0, values, size=n, dtype=np.uint64) if values == 256 else rng.integers(0, values, size=n, dtype=np.uint64) * U64(0x5B) + U64(0x11)
        keys = (keys & ~(U64(0xFF) << U64(8 * d))) | (byte << U64(8 * d))
    return keys


def full_random(n, rng):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64)


def live_digits(live, values=256):
    return lambda n, rng: _with_digits(n, rng, live, values)


def all_equal(key):
    return lambda n, rng: np.full(n, key, dtype=U64)


def one_differs(where, digit):
    """n - 1 equal keys and one that differs from them in one bit of `digit`, at the first, the last or the middle position."""

    def make(n, rng):
        keys = np.full(n, FILLED, dtype=U64)
        if n:
            keys[{"first": 0, "last": n - 1, "middle": n // 2}[where]] ^= U64(1) << U64(8 * digit)
        return keys

    return make


def two_keys_99_to_1(n, rng):
    a, b = U64(0x0123456789ABCDEF), U64(0xFEDCBA9876543210)  # (they differ in every digit: eight passes, one bucket nearly full in each)
    return np.where(rng.random(n) < 0.01, a, b).astype(U64)


def already_sorted(n, rng):
    return np.sort(full_random(n, rng))


def strictly_reverse_sorted(n, rng):
    steps = rng.integers(1, 1 << 44, size=n, dtype=np.uint64)  # (300 000 steps stay below 2^63)
    return np.cumsum(steps, dtype=np.uint64)[::-1].copy()


def extremes(n, rng):
    """0, 1, 2^63 - 1, 2^63, 2^64 - 1, and keys from a pool of sixteen that differ from one another in bit 63 only."""
    named = _u64([0, 1, (1 << 63) - 1, 1 << 63, ONES])
    pool = rng.integers(0, 1 << 63, size=16, dtype=np.uint64)
    keys = pool[rng.integers(0, 16, size=n)] | (rng.integers(0, 2, size=n, dtype=np.uint64) << U64(63))
    pick = rng.random(n) < 0.5
    keys[pick] = named[rng.integers(0, 5, size=n)][pick]
    return keys


def _length_and_rank(n, rng):
    """(len + 1) << 32 | rank, what cs_order sorts: 3000 ranks, each with its own byte length of up to 300."""
    lens = rng.integers(0, 301, size=3000, dtype=np.uint64)
    lens[:2] = (0, 300)
    rank = rng.integers(0, 3000, size=n)
    return ((lens[rank] + U64(1)) << U64(32)) | rank.astype(U64)


def order_keys(n, rng):
    return _length_and_rank(n, rng)


def order_keys_descending(n, rng):
    return ~_length_and_rank(n, rng)


def order_keys_with_nulls(n, rng):
    keys = _length_and_rank(n, rng)
    r = rng.random(n)
    keys[r < 0.025] = U64(0)
    keys[(r >= 0.025) & (r < 0.05)] = U64(ONES)
    return keys


def tie_keys(n, rng):
    """(seven key bytes) << 8 | (cnt + 8), as k_tie_keys builds it: cnt in -8 .. 7 bytes of the key lie inside the chunk, the
    bytes beyond them are zero; a small alphabet (NUL in it) so that most keys have equals."""
    cnt = rng.integers(-8, 8, size=n)
    alphabet = _u64([0x00, 0x61, 0x62, 0xE9])
    k = np.zeros(n, dtype=U64)
    for i in range(7):
        byte = np.where(i < cnt, alphabet[rng.integers(0, 4, size=n)], U64(0)).astype(U64)
        k = (k << U64(8)) | byte
    return (k << U64(8)) | (cnt + 8).astype(U64)


# (five and seven live digits of eight cannot all lie apart: those sets keep a skipped digit between two live ones somewhere)
LIVE_SETS = {2: (1, 5), 3: (0, 3, 6), 4: (0, 2, 4, 6), 5: (0, 2, 4, 5, 7), 6: (0, 1, 3, 4, 6, 7), 7: (0, 1, 2, 4, 5, 6, 7)}


def _families():
    f = {"full_random": (full_random, True)}
    for d in range(8):
        f["live_digit_%d_of_256_values" % d] = (live_digits((d,), 256), False)
        f["live_digit_%d_of_2_values" % d] = (live_digits((d,), 2), False)
    for k, live in LIVE_SETS.items():
        f["%d_live_digits" % k] = (live_digits(live), False)
    f["all_equal_zero"] = (all_equal(0), False)
    f["all_equal_ones"] = (all_equal(ONES), False)
    f["all_equal_mixed"] = (all_equal(0x0123456789ABCDEF), False)
    for where in ("first", "last", "middle"):
        for digit, name in ((7, "top"), (0, "bottom")):
            f["one_differs_%s_in_the_%s_digit" % (where, name)] = (one_differs(where, digit), False)
    f["two_keys_99_to_1"] = (two_keys_99_to_1, True)
    f["already_sorted"] = (already_sorted, True)
    f["strictly_reverse_sorted"] = (strictly_reverse_sorted, True)
    f["extremes"] = (extremes, False)
    f["order_keys"] = (order_keys, False)
    f["order_keys_descending"] = (order_keys_descending, False)
    f["order_keys_with_nulls"] = (order_keys_with_nulls, False)
    f["tie_keys"] = (tie_keys, False)
    return f


FAMILIES = _families()  # name -> (generator, runs at the large sizes too)


def sizes(name):
    large = FAMILIES[name][1]
    return SMALL_N + (LARGE_N if large else []) + ([HUGE_N] if name == "full_random" else [])


def keys_of(name, n):
    """The keys of case (name, n): the same in every process."""
    rng = np.random.default_rng([zlib.crc32(name.encode()), n])
    keys = _u64(FAMILIES[name][0](n, rng))
    assert keys.shape == (n,)
    return keys


def items_of(name, n):
    """The payload: random int32 values, negatives among them (so that a payload that does not travel with its key shows)."""
    rng = np.random.default_rng([zlib.crc32(name.encode()), n, 1])
    return rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64).astype(np.int32)


def reference(keys, items):
    """-> (keys, items) in stable ascending unsigned key order."""
    perm = np.argsort(keys, kind="stable")
    return keys[perm], items[perm]


def digit(keys, d):
    return ((keys >> U64(8 * d)) & U64(0xFF)).astype(np.int64)


def live_digit_positions(keys):
    """The digits a pass runs for: those that take more than one value."""
    return [d for d in range(8) if len(keys) > 1 and (digit(keys, d) != digit(keys, d)[0]).any()]


def most_equal_digits(keys, d, span):
    """The largest count of one value of digit d inside one aligned span of `span` pairs of the INPUT, and that span's size.
    (For the first pass that runs the input order is the order the kernel sees; later passes see the same multiset per digit
    in another order, so this is only asked about a case's lowest live digit.)"""
    best, best_size = 0, 0
    dg = digit(keys, d)
    for lo in range(0, len(keys), span):
        part = dg[lo: lo + span]
        c = int(np.bincount(part, minlength=256).max())
        if c > best:
            best, best_size = c, len(part)
    return best, best_size
