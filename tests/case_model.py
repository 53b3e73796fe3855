"""A model of lower / upper on well-formed rows, written over CHARACTERS (Python str) with the tables of
tools/unicode_tables.build(), and the generators of the columns that tests/test_case_cpu.py and tests/test_gpu_case.py run:
every BMP character that keeps its UTF-8 width through the tile kernel's table patch, the ones that change it, and rows of
arbitrary bytes that the ORACLE reports as size-keeping (the only malformed rows whose tile-kernel output is ever kept).
Needs no GPU."""
import numpy as np

import chartype_model as m

BITS = {"lower": m.UPPER, "upper": m.LOWER}  # the flag bit of the characters an op maps (32: upper case, 64: lower case)
OPS = ["lower", "upper"]
FOUR_BYTE = ["\U00010400", "\U0001F600"]  # cased in Unicode / not; both above U+FFFF: the tables do not reach them


def width(cp):
    return 1 if cp < 0x80 else 2 if cp < 0x800 else 3 if cp < 0x10000 else 4


def case_row(op, row):
    """row: str or None -> str or None"""
    if row is None:
        return None
    flags, cases = m.tables()
    bit = BITS[op]
    return "".join(chr(cases[ord(ch)]) if ord(ch) <= 0xFFFF and flags[ord(ch)] & bit else ch for ch in row)


def case_column(op, rows):
    return [case_row(op, r) for r in rows]


_split = {}


def _bmp_split(op):
    if op not in _split:
        flags, cases = m.tables()
        bit = BITS[op]
        keep, change = [], []
        for cp in range(0x80, 0x10000):
            if 0xD800 <= cp <= 0xDFFF:
                continue
            (change if flags[cp] & bit and width(cases[cp]) != width(cp) else keep).append(cp)
        _split[op] = (keep, change)
    return _split[op]


def keepers(op):
    """the BMP code points 0x80..0xFFFF (no surrogates) that `op` leaves at their UTF-8 width: mapped or not"""
    return list(_bmp_split(op)[0])


def changers(op):
    """... that `op` maps to a character of another UTF-8 width"""
    return list(_bmp_split(op)[1])


def cased():
    """the non-ASCII code points with the upper or the lower flag"""
    flags = m.tables()[0]
    return [cp for cp in range(0x80, 0x10000) if flags[cp] & (m.UPPER | m.LOWER)]


# ---- well-formed columns (rows of str / None) ------------------------------------------------------------------------------
def singles(op):
    return [chr(cp) for cp in keepers(op)]


def embedded(op):
    return ["aZ" + chr(cp) + "Zq" for cp in keepers(op)]


def packed(op):
    """rows of 20, 21 and 22 consecutive keepers and no ASCII: characters straddle the 16-byte pieces and the bitmap's 32-bit
    words, and the odd row sizes (63 and 66 bytes in the three-byte range, 42 in the two-byte one) move a row's first byte
    through every position of a piece and of a word; every 50th row holds the two four-byte characters"""
    keep = keepers(op)
    rows = []
    for per in (20, 21, 22):
        for at in range(0, len(keep), per):
            s = "".join(chr(cp) for cp in keep[at:at + per])
            if len(rows) % 50 == 7:
                s = s[:5] + FOUR_BYTE[0] + s[5:] + FOUR_BYTE[1]
            rows.append(s)
    return rows


def with_nulls(rows):
    return [None if i % 37 == 0 else r for i, r in enumerate(rows)]


def changer_column(op):
    return [chr(cp) for cp in changers(op)]


# ---- arbitrary bytes that keep their size ------------------------------------------------------------------------------------
ASCII_POOL = b"abcXYZ 09.qQ"
HIGH_POOL = bytes.fromhex("C3 A9 89 E2 82 AC F0 9F 98 80 C4 B0 FF 80 E1 B8 BF C5 ED A0")
# A truncated character at a row's end reads as zero-filled and GROWS the row by a byte (row_ops.h: decode_at), so such a
# row keeps its size only beside a character that shrinks: U+0130 (to 'i' in lower) and U+017F (to 'S' in upper) make both
# ops size-keeping.  The kernel must not patch a character that runs past its row: the byte behind belongs to the NEXT row,
# here an ASCII row nothing else would rewrite.
TAILS = [bytes.fromhex(h) for h in ("C3", "C4", "C5", "E1", "E1 B8", "E2", "E2 82", "ED", "ED A0", "F0", "F0 9F", "F0 9F 98", "FF")]


def truncated_tails():
    rows = []
    for tail in TAILS:
        for lead in range(18):  # (the row's first byte at every position of a piece)
            rows.append(b"abcXYZ 09.qQabcXYZ"[:lead] + "İſ".encode() + b"Zq" + tail)
            rows.append(b"Zq09 aB")
    return rows


def is_utf8(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def size_keeping_bytes(seed, rows, oracle):
    """-> (kept rows of bytes, oracle's lower of them, oracle's upper of them): `rows` rows of 0..89 bytes, a byte from
    HIGH_POOL with probability 0.04 and from ASCII_POOL otherwise, then truncated_tails(); kept when the ORACLE's lower and
    upper both leave the row at its size"""
    import cpulibs

    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 90, rows)
    total = int(lens.sum())
    high = rng.random(total) < 0.04
    a = np.frombuffer(ASCII_POOL, dtype=np.uint8)[rng.integers(0, len(ASCII_POOL), total)]
    h = np.frombuffer(HIGH_POOL, dtype=np.uint8)[rng.integers(0, len(HIGH_POOL), total)]
    data = np.where(high, h, a).astype(np.uint8).tobytes()
    cand, k = [], 0
    for ln in lens.tolist():
        cand.append(data[k:k + ln])
        k += ln
    cand += truncated_tails()
    col = cpulibs.Col.from_list(cand)
    low, up = oracle.lower(col), oracle.upper(col)
    n = np.diff(col.offsets)
    keep = np.flatnonzero((np.diff(low.offsets) == n) & (np.diff(up.offsets) == n)).tolist()
    low_rows, up_rows = low.to_bytes_list(), up.to_bytes_list()
    kept = [cand[i] for i in keep]
    kept_low = [low_rows[i] for i in keep]
    kept_up = [up_rows[i] for i in keep]
    malformed = [i for i, r in enumerate(kept) if not is_utf8(r)]
    assert len(malformed) >= 1000, len(malformed)
    # (bytes.lower() flips the ASCII letters and nothing else: what the kernel's piece lanes leave behind)
    assert sum(kept_low[i] != kept[i].lower() for i in malformed) >= 1000
    return kept, kept_low, kept_up
