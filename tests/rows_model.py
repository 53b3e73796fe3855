"""A plain model of find / contains / strip, a restatement of the staged-row tile plan from a column's offsets, and the
generators of the columns that tests/test_rows_model_cpu.py, tests/test_gpu_find_tile.py and tests/test_gpu_strip_tile.py run
through k_find_tile and k_strip_tile (custrings_amd/csrc/cs_rows.hip).  Needs no GPU, and nothing compiled from row_ops.h.

The model.  A row that is valid UTF-8 is a Python str and the operations are str.find / str.strip: positions, windows and
set members are characters.  For the other rows the reference's source decides (cpp/src/custring_view.inl), and its rules
are restated on bytes:
  * a character is a byte that is no continuation byte (10xxxxxx); the character position of a hit is the count of such
    bytes in front of it (char_offset, :1793);
  * the byte offset of character position k (offset_for_char_pos, :261) is 0 for k = 0, the row's size for k >= the row's
    characters, and otherwise THE SUM OF THE WIDTHS THE FIRST k LEAD BYTES ANNOUNCE -- whether the bytes behind a lead byte
    are its continuation bytes or not.  (The issue's "the window bounds are converted the same way" is the offset of the
    k-th lead byte; the oracle disagreed on rows like C3 C3 A9 'a' 'b', where position 2 -- the 'a' at byte 3 -- is byte 4, and the
    source decides.  A row with as many characters as bytes takes position k as byte k.)
    A row of continuation bytes alone has no characters: its window ends at position 0, byte 0, and neither find nor
    contains sees anything in it.  A window's END beyond the row's size makes the reference compare bytes behind the row: find() refuses such a call
    (Undefined), and the columns of arbitrary bytes are searched with windows that end behind every row;
  * strip (:1398-1598) decodes a character at the walk's position with the bytes past the row read as 0, walks the left end
    forward by the widths of the members it meets, and the right end back over the continuation bytes to the lead byte in
    front; it takes the decoded character's WIDTH off the right end, not the bytes walked over, so stray continuation
    bytes behind a member stay counted as kept.  lead + trail beyond the row's size is the empty row."""
import collections

import numpy as np

CONT = bytes(range(0x80, 0xC0))
DEFAULT_SET = " \n\t"


class Undefined(ValueError):
    """the reference reads bytes behind the row here"""


def nchars(b):
    return len(b.translate(None, CONT))


def lead_width(x):
    return 0 if (x & 0xC0) == 0x80 else 1 + (x >= 0xC0) + (x >= 0xE0) + (x >= 0xF0)


def as_text(b):
    try:
        return b.decode("utf-8")
    except UnicodeDecodeError:
        return None


def char_offset(row, k):
    """the byte offset of character position k, by the reference's table of widths"""
    if k <= 0:
        return 0
    n = nchars(row)
    if k >= n:
        return len(row)
    if n == len(row):
        return k
    off = seen = 0
    for x in row:
        w = lead_width(x)
        if w:
            if seen == k:
                break
            off += w
            seen += 1
    return off


def find(row, needle, start=0, end=-1):
    """row: bytes or None, needle: bytes -> character position, -1, or -2 for a null row"""
    if row is None:
        return -2
    if not needle:
        return -1
    start = max(start, 0)
    count = end - start
    text, sub = as_text(row), as_text(needle)
    if text is not None and sub is not None:
        return text.find(sub, start) if count < 0 else text.find(sub, start, start + count)
    total = nchars(row)
    lo = char_offset(row, start)
    hi = char_offset(row, total if count < 0 else min(start + count, total))  # (a row of continuation bytes alone: position 0, byte 0)
    if hi > len(row):
        raise Undefined((row, start, end))
    m = row.find(needle, lo, hi)  # (the hit wholly inside [lo, hi); lo beyond the row: none)
    return -1 if m < 0 else nchars(row[:m])


def contains(row, needle):
    return int(row is not None and len(needle) > 0 and needle in row and nchars(row) > 0)


def find_column(rows, needle, start=0, end=-1):
    """-> (int32 results, the count the entry returns: results != -1, null rows included)"""
    memo = {}
    out = np.empty(len(rows), dtype=np.int32)
    for i, r in enumerate(rows):
        if r not in memo:
            memo[r] = find(r, needle, start, end)
        out[i] = memo[r]
    return out, int(np.count_nonzero(out != -1))


def contains_column(rows, needle):
    out = np.array([contains(r, needle) for r in rows], dtype=np.uint8)
    return out, int(np.count_nonzero(out))


def _decode(row, i):
    """the character at byte i, bytes past the row read as 0 -> (its bytes, width); a continuation byte: itself, width 0"""
    if i >= len(row):
        return b"\0", 1
    w = lead_width(row[i])
    if w == 0:
        return row[i:i + 1], 0
    return (row[i:i + w] + b"\0\0\0")[:w], w


def strip(row, chars=None, side=0):
    """side 0: both ends, 1: the left, 2: the right; chars: str, None = the default set; members are characters"""
    if row is None:
        return None
    members = DEFAULT_SET if chars is None else chars
    text = as_text(row)
    if text is not None:
        return (text.strip(members), text.lstrip(members), text.rstrip(members))[side].encode()
    mem = set(ch.encode() for ch in members)
    n, count = len(row), nchars(row)
    lead = trail = 0
    if side != 2:
        for _ in range(count):
            ch, w = _decode(row, lead)
            if ch not in mem:
                break
            lead += w
        if lead == n:
            return b""
    if side != 1:
        p = n
        for _ in range(count):
            p -= 1
            while lead_width(row[p]) == 0:
                p -= 1
            ch, w = _decode(row, p)
            if ch not in mem:
                break
            trail += w
    if lead + trail > n:
        return b""
    return row[lead:n - trail]


def strip_column(rows, chars=None, side=0):
    memo = {}
    out = []
    for r in rows:
        if r not in memo:
            memo[r] = strip(r, chars, side)
        out.append(memo[r])
    return out


# ---- the column of a test: rows of bytes, null rows that may hold bytes ---------------------------------------------------
class Column:
    """rows: bytes or None; held: {row: the bytes a null row spans in the chars buffer}; want: the (R, route) the column
    was built for, per op -- check_plan() holds the column to it"""

    def __init__(self, rows, want_find=None, want_strip=None, held=None):
        self.rows = list(rows)
        self.held = dict(held or {})
        assert all(self.rows[i] is None for i in self.held)
        self.want = {"find": want_find, "strip": want_strip}

    def spans(self):
        return [self.held.get(i, b"") if r is None else r for i, r in enumerate(self.rows)]

    def offsets(self):
        offs = np.zeros(len(self.rows) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in self.spans()], out=offs[1:])
        return offs

    def col(self):
        import cpulibs

        chars = np.frombuffer(b"".join(self.spans()), dtype=np.uint8)
        valid = np.packbits(np.array([r is not None for r in self.rows], dtype=np.uint8), bitorder="little")
        return cpulibs.Col(chars, self.offsets(), valid)

    def check_plan(self, base=0):
        for op, want in self.want.items():
            if want is not None:
                p = plan(self.offsets(), op, base)
                assert (p.R, p.route) == want, (op, p.R, p.route, want)
        return self


# ---- the plan: plan_row_tiles / plan_staged_tiles of cs_plan.hip from the offsets alone -------------------------------------
PF_BYTES = 6144     # cstile::kPfBytes: what a wave's prefetch registers hold
PLAN_SLACK = 32     # plan_staged_tiles asks plan_row_tiles for span + 32 <= kPfBytes
STAGE_SLACK = 48    # cstile::kStageSlack: cap = the widest span + 48, rounded up to 16
Plan = collections.namedtuple("Plan", "R route cap ntiles spans oversize")


def tile_spans(offsets, R):
    offs = np.asarray(offsets, dtype=np.int64)
    rows = len(offs) - 1
    starts = np.arange(0, rows, R)
    return offs[np.minimum(starts + R, rows)] - offs[starts], offs[starts]


def plan(offsets, op, base=0):
    """op "find": R = 0 and route "rows" when no tile size fits; op "strip": 64-row tiles then, the ones beyond the staging
    buffer listed in `oversize` (span + lead + 48 > cap, lead = the address of the tile's first byte mod 16, `base` the
    address of the chars mod 16)"""
    rows = len(offsets) - 1
    if rows == 0:
        return Plan(0, "rows", 0, 0, [], [])
    for R in (64, 32, 16):
        spans, g0 = tile_spans(offsets, R)
        span = int(spans.max())
        if span + PLAN_SLACK <= PF_BYTES:
            break
    else:
        if op == "find":
            return Plan(0, "rows", 0, 0, [], [])
        R, span = 64, PF_BYTES - 64
        spans, g0 = tile_spans(offsets, R)
    cap = (span + STAGE_SLACK + 15) & ~15
    lead = (g0 + base) & 15
    over = np.flatnonzero(spans + lead + STAGE_SLACK > cap).tolist() if op == "strip" else []
    return Plan(R, "tile", cap, len(spans), spans.tolist(), over)


def find_route(col, needle):
    """the route cs_find / cs_contains must report for this column and needle"""
    if len(col.rows) == 0 or len(needle) > 64:
        return "rows"
    return plan(col.offsets(), "find").route


def wave_ranges(ntiles, workgroups):
    """RowTileWalk's split: the launch has min(workgroups, ceil(ntiles / 4)) workgroups of four waves, wave w walks the tiles
    [w * per, (w + 1) * per), per = ceil(ntiles / waves)"""
    waves = 4 * min(workgroups, (ntiles + 3) // 4)
    per = -(-ntiles // waves)
    return [(w * per, min(ntiles, (w + 1) * per)) for w in range(waves) if w * per < ntiles]


# ---- find / contains: the columns -------------------------------------------------------------------------------------------
FILL = b"x"
LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96]
HITS = [0, 1, 30, 31, 32, 33, 62, 63, 64, 65]
STARTS = [-3, 0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 200]
NEEDLE_SIZES = [1, 2, 3, 16, 63, 64]


def ascii_needle(nb):
    """'a' * (nb - 1) + 'b': every 'a' of a run of them is a candidate, the needle itself is where the run ends"""
    return b"a" * (nb - 1) + b"b" if nb > 1 else b"a"


def edge_rows(needle):
    """ASCII rows of the sizes around the needle's and around the 32-bit words of the candidate bitmap: without an
    occurrence, with the only one at the word boundaries and at the row's end, with the needle's first byte everywhere and
    the needle at the end, and with an occurrence that would need the first byte of the NEXT row"""
    nb = len(needle)
    rows = []
    for n in sorted(set(LENGTHS + [nb - 1, nb, nb + 1])):
        if not 0 <= n <= 96:
            continue
        rows.append(FILL * n)
        for p in sorted(set(HITS + [n - nb])):
            if 0 <= p and p + nb <= n:
                rows.append(FILL * p + needle + FILL * (n - p - nb))
        if n >= nb:
            rows.append(needle[:1] * (n - nb) + needle)
        if n >= nb - 1:
            rows.append(FILL * (n - nb + 1) + needle[:-1])
            rows.append(needle[-1:] + FILL * 2)
    return rows


def windows_for(needle):
    """(start, end): every start of STARTS with an inverted and an empty window, and with windows that end one byte short
    of, exactly at, and one byte behind the end of the first hit position at or behind the start and of the last one"""
    nb = len(needle)
    out = []
    for s in STARTS:
        ends = {s - 1, s}
        behind = [p for p in HITS if p >= max(s, 0)] or [HITS[-1]]
        for p in (behind[0], HITS[-1], 96 - nb):
            ends |= {p + nb - 1, p + nb, p + nb + 1}
        out += [(s, e) for e in sorted(ends)]
    return out


def col_edges(needle):
    return Column(edge_rows(needle), want_find=(64, "tile")).check_plan()


def col_mixed_tiles(needle):
    """the edge rows three times over, an 'é' row in every third 64-row tile: tiles of the windowed bit path next to
    tiles that walk their rows in LDS"""
    rows = edge_rows(needle) * 3
    rows += [FILL * 7] * (-len(rows) % 192)
    assert len(rows) >= 6 * 64
    for t in range(0, len(rows) // 64, 3):
        rows[t * 64 + 5] = "xé".encode() + needle
    return Column(rows, want_find=(64, "tile")).check_plan()


def col_one_long_row(needle):
    """64 rows of at most 96 bytes but one of 97: the tile leaves the bit path; the tile behind it takes it"""
    rows = edge_rows(needle)[-100:]
    rows[10] = FILL * (97 - len(needle)) + needle
    assert len(rows[10]) == 97 and max(len(r) for i, r in enumerate(rows) if i != 10) <= 96
    return Column(rows, want_find=(64, "tile")).check_plan()


MULTI_NEEDLES = ["é", "ü", "€", "😀", "aé"]


def col_multibyte(needle):
    """characters of 2, 3 and 4 bytes in front of the hit, the hit at byte offsets up to 90: the character position takes
    the continuation bits of one, two and three words.  In front of 'ü' stand 'é's: the same lead byte, a false candidate
    each."""
    text = needle.decode()
    rows = []
    for ch in ("é", "ü", "€", "😀", "é€😀"):
        if ch in text or text in ch:
            continue
        w = len(ch.encode())
        for k in range(0, 96 // w + 1):
            for pad in ("", "a", "zz"):
                r = (ch * k)[:k] + pad + text + "z"
                if len(r.encode()) <= 96:
                    rows.append(r.encode())
    assert max(r.index(needle) for r in rows) > 64 and any(32 < r.index(needle) <= 64 for r in rows)
    return Column(rows, want_find=(64, "tile")).check_plan()


SPARSE = [b"b", b"ab", b"ba", b"aab", b"bbbab", b"a", b"bb"]


def col_dense_then_sparse(workgroups):
    """32-row tiles (64 rows of 96 bytes do not fit) in the order D D S D D N: D 96-byte rows of 'a' (every bit of the tile's
    candidate bitmap set), S rows of 1 to 5 bytes, N null and empty rows; halfway one more S, so that D-S and D-N both fall
    inside a pair of tiles whatever a pair's first tile is.  The sparse tile writes a few 16-bit pieces of the bitmap and
    the null tile none: the dense tile's bits stay behind in LDS.  A wave walks consecutive tiles only when the launch has
    fewer waves than tiles: more than 4 * workgroups tiles with `workgroups` workgroups resident
    (CS_STREAM_BLOCKS_PER_CU=1: one a compute unit, 256 on the MI355X -- 1,033 tiles, 33,056 rows, which is why this column
    is beyond 20,000 rows)."""
    half = -(-(4 * workgroups + 4) // 12)
    kinds = list("DDSDDN") * half + ["S"] + list("DDSDDN") * half
    rows = []
    for t, kind in enumerate(kinds):
        if kind == "D":
            rows += [b"a" * 96] * 32
        elif kind == "S":
            rows += [SPARSE[(t + i) % len(SPARSE)] for i in range(32)]
        else:
            rows += [None if i % 2 else b"" for i in range(32)]
    c = Column(rows, want_find=(32, "tile")).check_plan()
    p = plan(c.offsets(), "find")
    assert p.ntiles == len(kinds) > 4 * workgroups
    seams = {kinds[t] + kinds[t + 1] for a, b in wave_ranges(p.ntiles, workgroups) for t in range(a, b - 1)}
    assert {"DS", "DN"} <= seams, seams  # some wave walks from a dense tile into a sparse one, and one into a null one
    return c


def _ascii_rows(n, lo, hi, needle, seed):
    """n rows of lo..hi bytes over "abx ", the needle dropped into every third one"""
    rng = np.random.default_rng(seed)
    rows = []
    for i, size in enumerate(rng.integers(lo, hi + 1, n).tolist()):
        r = bytes(rng.choice(np.frombuffer(b"abx ", dtype=np.uint8), size).tolist())
        if i % 3 == 0 and size >= len(needle):
            at = int(rng.integers(0, size - len(needle) + 1))
            r = r[:at] + needle + r[at + len(needle):]
        rows.append(r)
    return rows


def col_find_shape(shape, n, needle=b"ab", seed=3):
    """R64: rows up to 90 bytes; R32: every row 96 bytes (64 x 96 + 32 > 6144), still the bit path -- 190 bytes below 64 rows,
    and never below 33, where the first 32-row tile IS the first 64-row tile; R16: clusters of 32 rows of 250 bytes among
    short rows (the bit path next to the walk); rows: 32 rows of 400 bytes, no sixteen of which fit"""
    if shape == "R64":
        rows, want = _ascii_rows(n, 0, 90, needle, seed + n), (64, "tile")
    elif shape == "R32":
        assert n > 32
        size = 96 if n >= 64 else 190
        rows, want = _ascii_rows(n, size, size, needle, seed + n), (32, "tile")
    elif shape == "R16":
        rows = _ascii_rows(n, 0, 60, needle, seed + n)
        for at in range(0, n - 32, 200):
            rows[at:at + 32] = _ascii_rows(32, 250, 250, needle, seed + at)
        want = (16, "tile")
    else:
        rows = _ascii_rows(n, 0, 60, needle, seed + n)
        rows[n // 2:n // 2 + 32] = _ascii_rows(32, 400, 400, needle, seed)
        want = (0, "rows")
    assert len(rows) == n
    return Column(rows, want_find=want).check_plan()


ROW_COUNTS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513]  # 513: 9 tiles of 64 or 17 of 32 rows -- the last workgroup has one wave

MALFORMED_POOL = list(b"ab1.2 3.4.5.6 x9_\t\n") + [0, 0xC3, 0xA9, 0xE2, 0x82, 0xFF, 0x80, 0x1F] + [0xF0, 0x9F, 0x98, 0x80]
MALFORMED_NEEDLES = [b"a", b"3.4", "é".encode(), b"\xa9", b"\x80\xc3\xa9"]
# whole row and three windows.  The windows END behind every row (a row has at most 94 characters): an end inside a
# malformed row can lie behind the row's bytes by the reference's width sums, where it compares memory that is no row's.
MALFORMED_WINDOWS = [(0, -1), (1, 200), (9, 4), (33, 500)]


def col_malformed(rows=20_000, seed=11):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 95, rows)
    pool = np.array(MALFORMED_POOL, dtype=np.uint8)
    data = pool[rng.integers(0, len(pool), int(lens.sum()))].tobytes()
    null = rng.random(rows) <= 0.02
    out, held, k = [], {}, 0
    for i, ln in enumerate(lens.tolist()):
        if null[i]:
            out.append(None)
            held[i] = data[k:k + ln]
        else:
            out.append(data[k:k + ln])
        k += ln
    return Column(out, want_find=(64, "tile"), want_strip=(64, "tile"), held=held).check_plan()


# ---- strip: the sets and the columns ------------------------------------------------------------------------------------------
def _chars(first, n):
    return "".join(chr(first + i) for i in range(n))


SETS = {
    "default": None,
    "space": " ",
    "ab_": "ab ",
    "e_acute_": "é ",
    "euro_grin_tab": "€😀\t",
    "five": "ab cd",         # in_set: the ASCII bitmap from five members on
    "four": "ab c",          # ... the walk over c[] up to four
    "n64": _chars(0x100, 64),                                               # 64 non-ASCII members: the inline ones, all of them
    "n65": _chars(0x100, 65),                                               # one beyond: `wide`, one member in `more`
    "n200": _chars(0x100, 100) + " \tab" + _chars(0x4E00, 60) + _chars(0x1F600, 36),  # the binary search in `more`
}
MALFORMED_SETS = ["default", "ab_", "e_acute_", "five", "n65"]


def members_of(name):
    """a few members of the set, the last ones first: of a wide set those are in `more`"""
    s = DEFAULT_SET if SETS[name] is None else SETS[name]
    return [s[-1], s[0], s[len(s) // 2], s[-2]] if len(s) > 3 else list(s)


OUTSIDE = ["x", "ü", "Z9", "q₤q"]  # no set holds these ('ü' shares its lead byte with 'é' and with U+0100...: C3 / C4, '₤' two bytes with '€')


def strip_rows(name):
    """nothing to strip, the left only, the right only, both, stripped to nothing, a single member, a member kept inside,
    the empty row, a row ending in a cut character in front of a row that begins with continuation bytes"""
    m = members_of(name)
    rows = []
    for core in OUTSIDE + ["x" + m[0] + "x", "ü" + m[-1] + m[0] + "ü", "x" * 40]:
        for left in ("", m[0], m[0] + m[-1], "".join(m) * 2):
            for right in ("", m[-1], m[1 % len(m)] + m[0], "".join(reversed(m)) * 3):
                rows.append((left + core + right).encode())
    rows += [ch.encode() for ch in m] + ["".join(m).encode(), ("".join(m) * 9).encode(), b""]
    a = m[0].encode()
    for cut in {"é".encode(), "€".encode(), max(m, key=lambda ch: len(ch.encode())).encode()}:
        if len(cut) > 1:
            rows += [a + b"x" + cut[:-1], cut[-1:] + a + b"x" + a, cut + b"x" + cut + cut[:1], cut[1:] + cut, a + cut[:1], cut[1:] + a]
    return rows


def with_null_rows(rows, held_bytes=b" x "):
    """every 11th row null; every 22nd null row spans bytes of the chars buffer"""
    out, held = [], {}
    for i, r in enumerate(rows):
        if i % 11 == 5:
            out.append(None)
            if i % 22 == 5:
                held[i] = held_bytes
        else:
            out.append(r)
    return out, held


def col_strip_rows(name):
    rows, held = with_null_rows(strip_rows(name) * 2)
    return Column(rows, want_strip=(64, "tile"), held=held).check_plan()


STRIP_SHAPES = {"R64": (0, 40), "R32": (100, 180), "R16": (200, 370)}


def col_strip_shape(shape, n, name="e_acute_", seed=5):
    """rows sized for 64-, 32- and 16-row tiles, members of the set at both ends, a partial last tile"""
    lo, hi = STRIP_SHAPES[shape]
    m = members_of(name)
    rng = np.random.default_rng(seed + n)
    rows = []
    for size in rng.integers(lo, hi + 1, n).tolist():
        left = "".join(m[k] for k in rng.integers(0, len(m), int(rng.integers(0, 4))).tolist())
        right = "".join(m[k] for k in rng.integers(0, len(m), int(rng.integers(0, 4))).tolist())
        core = "".join(("x", "ü", m[0], "q ", "Z")[k] for k in rng.integers(0, 5, max(size, 1)).tolist())
        core = core.encode()[:max(size - len((left + right).encode()), 0)].decode("utf-8", "ignore")
        r = (left + core + right).encode()
        rows.append(r + b"x" * (lo - len(r)) if len(r) < lo else r)
    rows, held = with_null_rows(rows)
    assert n % int(shape[1:]) != 0
    return Column(rows, want_strip=(int(shape[1:]), "tile"), held=held).check_plan()


def col_strip_alignment(k, name="ab_"):
    """the first 64-row tile strips to k bytes and multiples of 16, so the second tile's output starts at k mod 16; then a
    full tile, a tile that strips to nothing, a full one, and a last tile of nothing"""
    m = members_of(name)
    pad = m[0].encode()
    first = [pad + b"q" * k + pad * 2] + [(pad * (i % 3) + b"0123456789ABCDEF" * (i % 4) + pad) for i in range(63)]
    full = [pad * (i % 5) + b"row %03d" % i + pad * (i % 2) for i in range(64)]
    nothing = [(pad * (i % 7), b"", None)[i % 3] for i in range(64)]
    rows = nothing + first + full + nothing + full + nothing[:41] if k == 0 else first + full + nothing + full + nothing[:41]
    c = Column(rows, want_strip=(64, "tile")).check_plan()
    out = strip_column(rows, SETS[name], 0)
    sizes = [sum(len(r or b"") for r in out[t:t + 64]) for t in range(0, len(rows), 64)]
    assert 0 in sizes and sum(sizes[:(2 if k == 0 else 1)]) % 16 == k, (k, sizes)
    return c


LONG = 7000


def col_strip_oversize(name="e_acute_"):
    """a 7,000-byte row leaves no tile size: 64-row tiles, the ones beyond the staging buffer copied from memory -- a row
    of up to 256 bytes by its lane, a longer one by the whole wave.  The first tile holds rows that strip to 255, 256,
    257 and 7,000 bytes, a long row that strips to nothing, a null row that spans bytes and an empty row; a middle tile a long
    row of 4-byte characters beside a 257-byte one; the last, partial tile three long rows."""
    m = members_of(name)
    a, z = m[0].encode(), m[-1].encode()
    short = [a * (i % 3) + b"r%d" % i + z * (i % 2) for i in range(64 * 5 + 9)]
    rows = list(short)
    held = {}

    def core(n):
        return b"x" + "ü".encode() * ((n - 2) // 2) + b"y" * (n % 2) + b"x"

    rows[3:10] = [a * 2 + core(255) + z, core(256) + z * 3, a + core(257), a * 5 + core(LONG) + z * 2, (a + z) * 3300, None, b""]
    held[8] = a + b"null" + z
    rows[64 * 2 + 31] = z + "😀".encode() * (LONG // 4) + a
    rows[64 * 2 + 32] = a + core(257) + a
    rows[64 * 5 + 1] = core(LONG)
    rows[64 * 5 + 2] = a * 300 + core(300) + z * 300
    rows[64 * 5 + 8] = z + core(257) + z
    c = Column(rows, want_strip=(64, "tile"), held=held).check_plan()
    p = plan(c.offsets(), "strip")
    assert p.oversize == [0, 2, 5] and p.ntiles == 6, p.oversize
    assert plan(c.offsets(), "find").route == "rows"
    out = strip_column(rows, SETS[name], 0)
    assert [len(out[i]) for i in (3, 4, 5, 6, 7)] == [255, 256, 257, LONG, 0]
    return c


# ---- the cases of the CPU and the GPU tests: what runs, and the route it must take ----------------------------------------------
MI355X_WORKGROUPS = 256  # one resident workgroup a compute unit under CS_STREAM_BLOCKS_PER_CU=1

FindCase = collections.namedtuple("FindCase", "name build needle windows route")
StripCase = collections.namedtuple("StripCase", "name build set_name sides route")
NEEDLE65 = ascii_needle(65)
SHAPE_COUNTS = [("R64", n) for n in ROW_COUNTS] + [("R32", n) for n in [33] + ROW_COUNTS if n > 32] + [("R16", 1000), ("rows", 1000)]


def find_cases():
    """name, the column's builder, the needle, the windows -- (0, -1) is the whole row -- and the route the table fixes"""
    cases = []
    for nb in NEEDLE_SIZES:
        nd = ascii_needle(nb)
        cases.append(FindCase("edges-%d" % nb, lambda nd=nd: col_edges(nd), nd, [(0, -1)] + windows_for(nd), "tile"))
    cases.append(FindCase("edges-65", lambda: col_edges(ascii_needle(64)), NEEDLE65, [(0, -1), (1, 90)], "rows"))
    for nb in (2, 16):
        nd = ascii_needle(nb)
        cases.append(FindCase("mixed-%d" % nb, lambda nd=nd: col_mixed_tiles(nd), nd, [(0, -1)] + windows_for(nd)[::4], "tile"))
    for nb in (2, 64):
        nd = ascii_needle(nb)
        cases.append(FindCase("one-long-row-%d" % nb, lambda nd=nd: col_one_long_row(nd), nd, [(0, -1), (1, 40), (33, 97), (64, 200)], "tile"))
    for text in MULTI_NEEDLES:
        nd = text.encode()
        cases.append(FindCase("multibyte-" + text, lambda nd=nd: col_multibyte(nd), nd, [(0, -1), (-3, -1), (0, 200), (5, 40), (33, 2)], "tile"))
    for shape, n in SHAPE_COUNTS:
        cases.append(FindCase("%s-%d" % (shape, n), lambda shape=shape, n=n: col_find_shape(shape, n), b"ab", [(0, -1), (3, 50)],
                              "rows" if shape == "rows" else "tile"))
    for nd in MALFORMED_NEEDLES:
        cases.append(FindCase("malformed-" + nd.hex(), col_malformed, nd, MALFORMED_WINDOWS, "tile"))
    return cases


def strip_cases():
    cases = []
    for name in SETS:
        cases.append(StripCase("rows-" + name, lambda name=name: col_strip_rows(name), name, (0, 1, 2), "tile"))
    for shape, n in (("R64", 64 * 3 + 7), ("R32", 32 * 5 + 9), ("R16", 16 * 7 + 3)):
        cases.append(StripCase("shape-" + shape, lambda shape=shape, n=n: col_strip_shape(shape, n), "e_acute_", (0, 1, 2), "tile"))
    for k in range(16):
        cases.append(StripCase("alignment-%d" % k, lambda k=k: col_strip_alignment(k), "ab_", (0,), "tile"))
    for name in ("e_acute_", "n200"):
        cases.append(StripCase("oversize-" + name, lambda name=name: col_strip_oversize(name), name, (0, 1, 2), "tile"))
    for name in MALFORMED_SETS:
        cases.append(StripCase("malformed-" + name, col_malformed, name, (0, 1, 2), "tile"))
    return cases
