"""The category key order on all three ordering routes of category_build (cs_category.hip), against plain Python over raw bytes.

    keys      = sorted(set(non-null rows))      Python's bytes order: unsigned, bytewise, shorter is less -- the contract at
                                                the head of cs_category.hip
    null key  = key 0 when any row is null
    values[r] = the index of row r's key (0 for a null row)

Key bytes, key offsets, the null key and every value are compared exactly.  Columns are built from raw bytes and int64
offsets, so rows hold NUL bytes and bytes that are no UTF-8.

Routes (switches, forwarded to the library by conftest.py):
    default              up to 2048 distinct keys: the compare network in one LDS chunk; beyond: the radix sort on the 8-byte
                         prefix, then the tied records by the network (up to 2048 of them) or by rounds of radix sorts
    CS_CAT_BITONIC=1     the compare network over all records
    CS_CAT_TIE_NETWORK=1 the radix sort on the prefix, then the network over all tied records

No route string reports which kernels ran; by `sort_network`, which category_build's ordering calls (kSortChunk = 2048): the network pads U
records to the next power of two P; for P > 2048 it runs k_bitonic_local on P / 2048 chunks for the stages k = 2 .. 2048,
then for every stage k = 4096 .. P one k_bitonic_step launch for each j = k / 2 .. 2048 and one k_bitonic_local tail
(j = 1024 .. 1).  So with CS_CAT_BITONIC the counts 2049 .. 4096 (P = 4096) launch k_bitonic_step once (k 4096, j 2048) and
4097, 6000 (P = 8192) three times (k 4096: j 2048; k 8192: j 4096, 2048); 2047 and 2048 stay in one chunk.  With
CS_CAT_TIE_NETWORK the same holds for the number of TIED records: all U for the key sets whose keys share their first 8 bytes
(shared_prefix, length_edges with one stem), a handful for random keys."""
import random

import numpy as np
import pytest

import gpuutil

pytestmark = pytest.mark.gpu

COUNTS = [2047, 2048, 2049, 4096, 4097, 6000]
ROWS = 9000
ROUTES = [("default", None), ("network", "CS_CAT_BITONIC"), ("tie_network", "CS_CAT_TIE_NETWORK")]


def _distinct(count, draw):
    keys = {}
    while len(keys) < count:
        keys[draw()] = None
    return list(keys)


def random_12_bytes(count, rnd):
    """Prefixes almost all distinct: few ties."""
    return _distinct(count, lambda: rnd.randbytes(12))


def shared_prefix(count, rnd):
    """One 16-byte prefix, random tails of 0 to 20 bytes: every record ties on the 8-byte prefix AND on the first 7-byte chunk
    (tie rounds beyond one), every compare of the network goes through compare_keys."""
    head = b"shared-16-bytes-"
    assert len(head) == 16
    return _distinct(count, lambda: head + rnd.randbytes(rnd.randrange(21)))


def prefix_chains(count, rnd):
    """Chains in which each key is a prefix of the next, up to 12 bytes: b"a", b"a\\0", b"a\\0\\0", ... (zero padding makes the
    8-byte prefixes and the 7-byte chunks of a chain equal: only the length decides), and chains that repeat another byte."""
    keys = {}

    def chain(head, fill):
        for k in range(13 - len(head)):
            keys[head + fill * k] = None

    chain(b"a", b"\0")
    chain(b"", b"\0")  # the empty key and runs of NUL
    while len(keys) < count:
        head = bytes([rnd.randrange(1, 256) for _ in range(rnd.randrange(1, 4))])
        chain(head, b"\0")
        chain(head, bytes([head[-1]]))
        chain(head, b"\xff")
    out = list(keys)[:count]
    assert all(k in out for k in (b"a", b"a\0", b"a\0\0", b"a" + b"\0" * 11, b"", b"\0"))
    return out


def sign_straddle(count, rnd):
    """Bytes 0x7F and 0x80 only: the first differing byte of any two keys straddles the sign bit."""
    return _distinct(count, lambda: bytes(rnd.choice((0x7F, 0x80)) for _ in range(rnd.randrange(1, 15))))


def length_edges(count, rnd):
    """Keys of exactly 7, 8, 9, 14, 15, 16, 21 and 22 bytes that share all but the last byte (the 8-byte prefix, the 7-byte chunks
    of the tie rounds and the 21 key bytes inside a table slot end there); a shorter stem is a prefix of the longer ones.  256
    last bytes a length: one stem gives 2048 keys, so larger counts take a second and a third stem."""
    keys = []
    for first in (b"s", b"t", b"\x80"):
        stem = first + b"tem\0stem-stem\xffstem-st"
        assert len(stem) == 22
        for n in (7, 8, 9, 14, 15, 16, 21, 22):
            keys += [stem[: n - 1] + bytes([b]) for b in range(256)]
    assert len(set(keys)) == len(keys) == 3 * 2048
    if count <= 2048:
        keys = keys[:2048]  # (one stem: every key shares the first 6 bytes)
    rnd.shuffle(keys)
    return keys[:count]


KEY_SETS = {"random_12_bytes": random_12_bytes, "shared_prefix": shared_prefix, "prefix_chains": prefix_chains, "sign_straddle": sign_straddle,
            "length_edges": length_edges}


def make_rows(keys, nulls, rnd):
    """ROWS rows, shuffled: every key once (the distinct count is exact), 5 % null rows when asked, the rest drawn at random from
    the keys (most keys repeat)."""
    rows = list(keys) + [None] * (ROWS // 20 if nulls else 0)
    rows += [rnd.choice(keys) for _ in range(ROWS - len(rows))]
    rnd.shuffle(rows)
    return rows


def column(rows):
    """The device column of `rows` (bytes or None) from raw chars, int64 offsets and a validity mask."""
    lens = np.array([0 if r is None else len(r) for r in rows], dtype=np.int64)
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    chars = np.frombuffer(b"".join(r for r in rows if r is not None) + b"\0", dtype=np.uint8)  # (never an empty buffer)
    validity = None
    if any(r is None for r in rows):
        validity = np.packbits(np.array([r is not None for r in rows], dtype=np.uint8), bitorder="little")
    from custrings_amd import nvstrings

    return nvstrings.from_offsets64(chars, offsets, len(rows), validity)


def reference(rows):
    """-> (keys in order, None first when a row is null; values)"""
    keys = sorted(set(r for r in rows if r is not None))
    if any(r is None for r in rows):
        keys = [None] + keys
    index = {k: i for i, k in enumerate(keys)}
    return keys, [index[r] for r in rows]


def check_category(rows, what):
    from custrings_amd import nvcategory

    want_keys, want_values = reference(rows)
    cat = nvcategory.from_strings(column(rows))
    chars, offs, valid = cat.keys()._export64()
    assert cat.keys_size() == len(want_keys), "%s: %d keys, expected %d" % (what, cat.keys_size(), len(want_keys))
    bits = np.unpackbits(valid, bitorder="little")[: len(want_keys)].astype(bool)
    assert bits.tolist() == [k is not None for k in want_keys], what + ": the null key"
    want_lens = [0 if k is None else len(k) for k in want_keys]
    want_offs = np.concatenate([[0], np.cumsum(want_lens)]).astype(np.int64)
    data = chars.tobytes()
    got_keys = [data[offs[i]: offs[i + 1]] if bits[i] else None for i in range(len(want_keys))]
    bad = [i for i, (a, b) in enumerate(zip(got_keys, want_keys)) if a != b]
    assert not bad, "%s: %d keys differ, the first at %d: %r, expected %r" % (what, len(bad), bad[0], got_keys[bad[0]], want_keys[bad[0]])
    assert np.array_equal(offs, want_offs), what + ": key offsets"
    assert data == b"".join(k for k in want_keys if k is not None), what + ": key bytes"
    values = np.asarray(cat.values(), dtype=np.int64)
    wrong = np.flatnonzero(values != np.asarray(want_values, dtype=np.int64))
    assert wrong.size == 0, "%s: %d values differ, the first at row %d: %d, expected %d" % (
        what, wrong.size, wrong[0], values[wrong[0]], want_values[wrong[0]])


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("kind", list(KEY_SETS))
def test_gpu_category_key_order_on_every_ordering_route(kind, count, monkeypatch):
    """`count` distinct keys drawn into 9000 rows, with 5 % nulls and without, on the three routes (the derivation of which
    kernels each count launches is at the head of this file)."""
    rnd = random.Random("%s %d" % (kind, count))
    keys = KEY_SETS[kind](count, rnd)
    assert len(set(keys)) == len(keys) == count
    for nulls in (False, True):
        rows = make_rows(keys, nulls, rnd)
        assert len(rows) == ROWS and len(set(r for r in rows if r is not None)) == count and (None in rows) == nulls
        for route, switch in ROUTES:
            for _, other in ROUTES:
                if other:
                    monkeypatch.delenv(other, raising=False)
            if switch:
                monkeypatch.setenv(switch, "1")
            check_category(rows, "%s, %d keys, %s, route %s" % (kind, count, "5 % nulls" if nulls else "no nulls", route))


# ---- the sampled sizing of the table --------------------------------------------------------------------------------------
# category_build's first table has 2^22 slots; after an overflow of a table of at least 2^22 slots, a column of more than
# 2^21 rows is sampled at a stride and the next table sized from the sample's share of distinct keys.  2^22 + 1 distinct keys
# cannot fit the first table whatever the hash does, and such a column has more than 2^21 rows: the smallest shape that must
# take the branch.  With these rows the table for all-distinct rows has 2^24 slots, and so have the sample's size and the
# 16-fold one: the second attempt is the unlimited one, in 32-byte slots.
BIG_ROWS = 4_300_000
BIG_NULLS = 3000
assert BIG_ROWS - BIG_NULLS > (1 << 22)

_big = {}


def big_distinct_rows(nulls):
    """-> (values, valid): BIG_ROWS distinct uint64 values in random order (a row's key is the value's eight big-endian bytes,
    so the key bytes vary in every position and the key order is the numeric order) and which rows are not null."""
    if "values" not in _big:
        rng = np.random.default_rng(20260422)
        values = rng.integers(0, 1 << 64, size=BIG_ROWS, dtype=np.uint64, endpoint=False)
        assert np.unique(values).size == BIG_ROWS
        valid = np.ones(BIG_ROWS, dtype=bool)
        valid[rng.choice(BIG_ROWS, size=BIG_NULLS, replace=False)] = False
        values.setflags(write=False)
        valid.setflags(write=False)
        _big["values"], _big["valid"] = values, valid
    return _big["values"], (_big["valid"] if nulls else np.ones(BIG_ROWS, dtype=bool))


def big_distinct_column(nulls):
    """The device column of big_distinct_rows from raw chars, int64 offsets and a validity mask (null rows hold no bytes)."""
    from custrings_amd import nvstrings

    values, valid = big_distinct_rows(nulls)
    chars = np.append(values[valid].astype(">u8").view(np.uint8), np.uint8(0))  # (never an empty buffer)
    offsets = np.zeros(BIG_ROWS + 1, dtype=np.int64)
    np.cumsum(8 * valid.astype(np.int64), out=offsets[1:])
    validity = None if valid.all() else np.packbits(valid.astype(np.uint8), bitorder="little")
    return nvstrings.from_offsets64(chars, offsets, BIG_ROWS, validity)


def big_distinct_expected(nulls):
    """-> (key bytes, key offsets, values) by numpy alone: the sorted values, the null key first when a row is null, and every
    row's rank."""
    values, valid = big_distinct_rows(nulls)
    shift = 0 if valid.all() else 1
    keys = np.sort(values[valid])
    offs = np.concatenate([np.zeros(1 + shift, dtype=np.int64), 8 * np.arange(1, keys.size + 1, dtype=np.int64)])
    ranks = np.where(valid, np.searchsorted(keys, values) + shift, 0).astype(np.int32)
    return keys.astype(">u8").view(np.uint8), offs, ranks


@pytest.mark.parametrize("nulls", [False, True], ids=["no_nulls", "nulls"])
def test_gpu_category_sampled_table_size(nulls):
    """4.3M rows, every one a distinct 8-byte key (and 3000 null rows mixed in): the first table overflows, the sample sizes the
    second.  Key bytes, key offsets, the null key and every value exactly, against numpy."""
    from custrings_amd import nvcategory

    want_chars, want_offs, want_values = big_distinct_expected(nulls)
    nkeys = want_offs.size - 1
    cat = nvcategory.from_strings(big_distinct_column(nulls))
    assert cat.keys_size() == nkeys
    chars, offs, valid = cat.keys()._export64()
    bits = np.unpackbits(valid, bitorder="little")[:nkeys].astype(bool)
    assert bits[0] == (not nulls) and bits[1:].all(), "the null key"
    assert np.array_equal(offs, want_offs), "key offsets"
    assert np.array_equal(chars, want_chars), "key bytes"
    values = np.full(BIG_ROWS, -1, dtype=np.int32)
    cat.values(values)
    wrong = np.flatnonzero(values != want_values)
    assert wrong.size == 0, "%d values differ, the first at row %d: %d, expected %d" % (wrong.size, wrong[0], values[wrong[0]], want_values[wrong[0]])
