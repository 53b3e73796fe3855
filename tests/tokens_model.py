"""A plain model of NVText tokenize (whitespace and delimiter-set mode) and create_ngrams, the restated choices of their tile
kernels -- tokenize's tile size and segments (cs_tokenize.hip), the n-grams a lane M of ngrams_fast (cs_ngram.hip) -- and the
generators of the columns that tests/test_tokens_model_cpu.py, tests/test_gpu_tokenize_tile.py and
tests/test_gpu_ngrams_tile.py run.  Needs no GPU and nothing compiled.

tokenize.  A row that is valid UTF-8 is a Python str: its tokens are the runs of characters that are no delimiters
(whitespace mode: a character above ' '; set mode: a character the delimiter string does not hold; NUL is a delimiter in
whitespace mode and never one in set mode).  For the other rows the reference's source decides (cpp/src/text/tokens.cu:41-121,
cpp/src/custring_view.inl), restated on bytes in walk():
  * the row has as many characters as bytes that are no continuation bytes (chars_in_string, :1758);
  * the iterator is a byte offset and a character position; ++ adds the width THE BYTE AT THE OFFSET announces (:361) -- 0
    for a continuation byte, on which the iterator stands still and which it then reads once for every character left --
    and * decodes that many bytes there (:1724; a continuation byte: itself);
  * a delimiter in set mode is what custring_view::find(Char) (:517) finds: it decodes the delimiter string at EVERY byte
    offset, so a member's continuation byte is found too, and the character 0 never;
  * the token's character positions become byte offsets by offset_for_char_pos (:261, rows_model.char_offset): the sum of
    the widths the first k lead bytes announce.
The byte AT the row's size is the reference's terminator, 0.  Undefined is raised where the reference reads a byte behind
that, where the bytes a decode reads behind the row decide whether the character is a delimiter, and where a token's byte
offsets do not lie inside the row in order.  walk(strict=False) is what the project does there: bytes behind the
row read as 0, a token ends at the row's end at the latest and one that would begin there is dropped.

Null rows span no bytes in any column the library takes (cs_column.hip makes a copied column canonical and refuses a
borrowed one that is not), so "null rows that span bytes" exist on the host side only: Column.held."""
import collections
import re

import numpy as np

import rows_model as rm
from rows_model import Column, Undefined, PF_BYTES

CONT = rm.CONT


# ---- tokenize: the model -----------------------------------------------------------------------------------------------------
def _is_delim(ch, delim):
    """ch: the decoded bytes; delim: None or the delimiter string's bytes"""
    if delim is None:
        return len(ch) == 1 and ch[0] <= 0x20
    if ch == b"\0":
        return False
    w = len(ch)
    for i in range(0, len(delim) - w + 1):
        wi = max(rm.lead_width(delim[i]), 1)
        if wi == w and delim[i:i + w] == ch:
            return True
    return False


def _behind_matters(seen, w, delim):
    """would bytes behind the row decide?  `seen`: the bytes of the character inside the row, w: its announced width"""
    if delim is None:
        return False  # (more than one byte: above ' ' whatever follows)
    return any(rm.lead_width(delim[i]) == w and delim[i:i + len(seen)] == seen for i in range(len(delim)))


def walk(row, delim=None, strict=True):
    """the reference's walk of one row that is not valid UTF-8 -> [(lo, hi)]"""
    n, nch = len(row), rm.nchars(row)
    out = []
    spaces, spos, epos, off, cpos = True, 0, nch, 0, 0

    def width_at(off):
        if off > n and strict:
            raise Undefined(row)
        return rm.lead_width(row[off]) if off < n else 1

    while spos < nch:
        while cpos != nch:
            w = width_at(off)
            ch = (row[off:off + max(w, 1)] if off < n else b"\0")
            if len(ch) < max(w, 1):
                if strict and _behind_matters(ch, w, delim):
                    raise Undefined(row)
                ch = ch + b"\0" * (w - len(ch))
            d = _is_delim(ch, delim)
            if spaces == d:
                if spaces:
                    spos = cpos + 1
                else:
                    epos = cpos + 1
            else:
                spaces = not spaces
                if spaces:
                    epos = cpos
                    break
            off += w
            cpos += 1
        if not spos < epos:
            break
        lo, hi = rm.char_offset(row, spos), rm.char_offset(row, epos)
        if strict and not lo < hi <= n:
            raise Undefined(row)
        lo, hi = min(lo, n), min(hi, n)
        if lo < hi:
            out.append((lo, hi))
        spos, epos = epos + 1, nch
        if spos >= nch:
            break  # (the reference's ++itr behind the last token reads a width nobody uses)
        off += width_at(off)
        cpos += 1
    return out


def tokens_of(row, delim=None, strict=True):
    """row: bytes, delim: None or str -> the row's tokens (bytes)"""
    text = rm.as_text(row)
    if text is not None:
        pat = "[^\\x00-\\x20]+" if delim is None else "[^" + re.escape(delim) + "]+"
        return [t.encode() for t in re.findall(pat, text)]
    return [row[lo:hi] for lo, hi in walk(row, None if delim is None else delim.encode(), strict)]


def tokenize_column(rows, delim=None, strict=True):
    """-> (the tokens of all rows in order, the rows the model calls Undefined: those contribute nothing)"""
    memo, out, undefined = {}, [], []
    for i, r in enumerate(rows):
        if r is None:
            continue
        if r not in memo:
            try:
                memo[r] = tokens_of(r, delim, strict)
            except Undefined:
                memo[r] = None
        if memo[r] is None:
            undefined.append(i)
        else:
            out += memo[r]
    return out, undefined


def malformed_rows(rows):
    return [i for i, r in enumerate(rows) if r is not None and rm.as_text(r) is None]


def ngrams(rows, n=2, sep=b"_"):
    """create_ngrams (ngram.cu:32-110): null and empty rows are dropped; no more rows left than n: join over ALL rows (a null
    row joins as ""); n == 1: the column"""
    n = n or 2
    if not rows:
        return []
    kept = [r for r in rows if r]
    if len(kept) <= n:
        return [sep.join(r or b"" for r in rows)]
    if n == 1:
        return list(rows)
    return [sep.join(kept[i:i + n]) for i in range(len(kept) - n + 1)]


# ---- the plans -----------------------------------------------------------------------------------------------------------------
SEG = PF_BYTES  # k_tok_tile's segment: cstile::kPfChunks * 1024 staged bytes
TokPlan = collections.namedtuple("TokPlan", "R route segs")


def tok_plan(offsets, base=0, outliers=True):
    """tokenize_fast's plan_row_tiles(col, 16): the first R of 64, 32, 16 whose widest tile + 16 fits the prefetch registers;
    none: 64-row tiles, the oversize ones in segments ("tile-segs"; "rows" under CS_NO_OUTLIER_TILES).  segs: the segments
    of every tile, from its span and the address of its first byte mod 16"""
    rows = len(offsets) - 1
    if rows == 0:
        return TokPlan(0, "rows", [])
    for R in (64, 32, 16):
        spans, g0 = rm.tile_spans(offsets, R)
        if int(spans.max()) + 16 <= PF_BYTES:
            return TokPlan(R, "tile", [1] * len(spans))
    if not outliers:
        return TokPlan(0, "rows", [])
    spans, g0 = rm.tile_spans(offsets, 64)
    want = spans + ((g0 + base) & 15)
    return TokPlan(64, "tile-segs", np.maximum(1, -(-want // SEG)).tolist())


def tok_route(rows, delim, base=0, outliers=True, offsets=None):
    """the route cs_tokenize must note: "rows" for more than four delimiters, a non-ASCII or empty set, and a column with a
    row that is not well-formed UTF-8 by the kernel's check (every lead byte followed by the continuation bytes it announces
    inside its row, no other continuation byte -- a wider notion than valid UTF-8: F8 80 80 80 passes)"""
    if delim is not None and (len(delim.encode()) > 4 or delim == "" or any(ord(c) >= 128 for c in delim)):
        return "rows"
    if any(r is not None and not well_formed(r) for r in rows):
        return "rows"
    offs = Column(rows).offsets() if offsets is None else offsets
    return tok_plan(offs, base, outliers).route


def well_formed(row):
    i, n = 0, len(row)
    while i < n:
        w = rm.lead_width(row[i])
        if w == 0 or i + w > n or any(rm.lead_width(x) != 0 for x in row[i + 1:i + w]):
            return False
        i += w
    return True


def ngram_m(offsets, n, sepn, m_first=8):
    """ngrams_fast's M for a column without null or empty rows: the first m of 8, 4, 2, 1 (from CS_NGRAM_M down) whose widest
    tile fits -- input span + 32 <= kPfBytes, output span + 64 <= 12 KB -- preferring, down to 4, one whose LDS leaves room
    for four workgroups (four waves' regions within 40 KB); 0: no m fits, or the call is not the tile kernel's"""
    offs = np.asarray(offsets, dtype=np.int64)
    rows = len(offs) - 1
    if n < 2 or n > 8 or sepn > 8 or rows <= n:
        return 0
    M = 0
    for m in (8, 4, 2, 1):
        if m > m_first:
            continue
        NG = 64 * m
        h0, h1 = ngram_spans(offs, n, sepn, m)
        if h0 + 32 <= PF_BYTES and h1 + 64 <= 12 * 1024:
            wave = (((NG + n + 1) * 4 + 15) & ~15) + ((h0 + 32 + 15) & ~15) + ((h1 + 64 + 15) & ~15)
            roomy = wave * 4 <= 40 * 1024
            if not M or roomy:
                M = m
            if roomy or m <= 4:
                break
    return M


def ngram_spans(offsets, n, sepn, m):
    """k_ngram_spans: the widest input and the widest output span of a tile of 64 * m n-grams"""
    offs = np.asarray(offsets, dtype=np.int64)
    ng, NG = len(offs) - n, 64 * m
    G0 = np.arange(0, ng, NG)
    ngt = np.minimum(NG, ng - G0)
    sin = offs[G0 + ngt + n - 1] - offs[G0]
    sout = ngt * (n - 1) * sepn + sum(offs[G0 + ngt + k] - offs[G0 + k] for k in range(n))
    return int(sin.max()), int(sout.max())


def or_bytes_calls(rows, n, sepn, m):
    """what k_ngram_tile hands or_bytes for the tokens of a column whose chars start at a 16-byte boundary:
    (source alignment si & 3, destination alignment di & 3, the token's bytes) for every token of every n-gram; the
    destination counts from the tile's first n-gram, the source from the 16-byte piece the tile's first token lies in"""
    offs = Column(rows).offsets()
    out = []
    ng, NG = len(rows) - n + 1, 64 * m
    for G0 in range(0, ng, NG):
        c0, di = int(offs[G0]), 0
        for g in range(G0, min(G0 + NG, ng)):
            for k in range(n):
                ln = int(offs[g + k + 1] - offs[g + k])
                out.append((((c0 & 15) + int(offs[g + k]) - c0) & 3, di & 3, ln))
                di += ln + (sepn if k + 1 < n else 0)
    return out


def toks_input_bound():
    """n = 2, no separator: at M = 2 a tile's INPUT span (three tokens of 400 bytes, 126 of 40) is beyond kPfBytes - 32 while
    its output span is within 12 KB - 64; M = 1 fits.  The other columns that force an M are bound by their output"""
    rows = [_token(i, 400 if i % 64 == 0 else 40) for i in range(64 * 3 + 2)]
    offs = Column(rows).offsets()
    (i2, o2), (i1, o1) = ngram_spans(offs, 2, 0, 2), ngram_spans(offs, 2, 0, 1)
    assert i2 + 32 > PF_BYTES and o2 + 64 <= 12 * 1024 and i1 + 32 <= PF_BYTES and o1 + 64 <= 12 * 1024, (i2, o2, i1, o1)
    return rows


def ngram_route(rows, n, sep, m_first=8):
    if any(not r for r in rows):
        return "rows"
    m = ngram_m(Column(rows).offsets(), n or 2, len(sep), m_first)
    return "tile-m%d" % m if m else "rows"


# ---- tokenize: the columns -----------------------------------------------------------------------------------------------------
WORDS = ["a", "bc", "déf", "x" * 17, "12.5", "😀", "tab\tbed", "q" * 40, "€uro", "_", "-x-", "."]
GAPS = [" ", "  ", "\n", "_", "-", " \t ", ".", ""]
SHAPES = {"R64": (64 * 3 + 7, 0, 40), "R32": (32 * 5 + 9, 100, 180), "R16": (16 * 7 + 3, 200, 370)}
SETS = [None, " ", " .", "_-", " _-."]  # whitespace, and one, two and four ASCII delimiters (three: "_- " below)
ROWS_SETS = ["abcde", "é "]            # five bytes; a non-ASCII member: the row-wise kernels


def _text_row(rng, size):
    t = GAPS[int(rng.integers(0, 3))]
    while len(t.encode()) < size:
        t += WORDS[int(rng.integers(0, len(WORDS)))] + GAPS[int(rng.integers(0, len(GAPS)))]
    return t.encode()[:size].decode("utf-8", "ignore").encode()


def col_tok_shape(shape, seed=7, nulls=True):
    """well-formed text sized for 64-, 32- and 16-row tiles with a partial last tile; null, empty and all-delimiter rows"""
    n, lo, hi = SHAPES[shape]
    rng = np.random.default_rng(seed + n)
    rows = [_text_row(rng, int(s)) for s in rng.integers(lo, hi + 1, n)]
    rows = [r + b"x" * (lo - len(r)) for r in rows]
    held = {}
    if nulls:
        for i in range(3, n, 29):
            rows[i] = (b"", b" \t \n", b"__--")[i % 3] if lo == 0 else rows[i]
        rows, held = rm.with_null_rows(rows)
    c = Column(rows, held=held)
    p = tok_plan(Column(rows).offsets())  # (null rows span nothing on the device)
    assert (p.R, p.route) == (int(shape[1:]), "tile") and n % p.R != 0, p
    return c


def col_tok_segs():
    """no tile size fits: 64-row tiles.  Tile 0 spans two segments and 300 bytes: row 1 ends at byte 6144 with a kept byte, row
    2 is empty AT the boundary (p - seg_lo == want for segment 0, == 0 for segment 1), row 3 opens a token there -- behind a
    kept byte, across segments -- and is a run of 'é' at an odd offset, which straddles every later 16-byte piece and chunk
    row; tile 1 is ordinary; tile 2 spans three segments with a 3-byte character across both boundaries, a token that begins
    at the first byte of segment 2 behind a delimiter, and a partial row count"""
    rng = np.random.default_rng(5)
    short = [_text_row(rng, int(s)) for s in rng.integers(0, 30, 64 * 2 + 5)]
    rows = list(short)
    rows[0] = b"ab cd" + b"x" * 95
    rows[1] = (b"word " * 1300)[:SEG - 100 - 1] + b"z"
    rows[2] = b""
    rows[3] = b"Q" + "é".encode() * 150 + b" t"
    for i in range(4, 64):
        rows[i] = b""
    assert sum(len(r) for r in rows[:2]) == SEG and sum(len(r) for r in rows[:64]) == SEG + 303
    start2 = sum(len(r) for r in rows[:128])
    lead = start2 & 15
    a = SEG - lead - 1  # the '€' of row 128 lies across the first boundary of tile 2
    rows[128] = b"y" * a + "€".encode() + b" " + b"k" * 100
    used = lead + len(rows[128])
    rows[129] = b"m" * (2 * SEG - used - 2) + b"n "  # a delimiter is the last byte of segment 1 ...
    rows[130] = b"T" + "€".encode() * 40                            # ... and a row and a token open segment 2
    assert lead + sum(len(r) for r in rows[128:130]) == 2 * SEG
    c = Column(rows)
    p = tok_plan(c.offsets())
    assert (p.R, p.route, p.segs) == (64, "tile-segs", [2, 1, 3]), p
    assert tok_plan(c.offsets(), outliers=False).route == "rows"
    return c


def lead_positions(rows, R=64):
    """(announced width, staged position inside its tile: lead + byte) of every lead byte of a multi-byte character, for a
    column whose chars start at a 16-byte boundary"""
    offs = Column(rows).offsets()
    out = []
    for t in range(0, len(rows), R):
        g0 = int(offs[t])
        for i in range(t, min(t + R, len(rows))):
            out += [(rm.lead_width(x), (g0 & 15) + int(offs[i]) - g0 + j) for j, x in enumerate(rows[i] or b"") if x >= 0xC0]
    return out


def col_tok_utf8_edges():
    """well-formed runs of 2-, 3- and 4-byte characters placed from the offsets: a lead byte of every width in each of the
    last bytes of a 1024-byte chunk row that still leave a continuation byte for the next one (carry_expect from lane 63:
    'é' at 1023, '€' at 1022 and 1023, a 4-byte character at 1021, 1022 and 1023 -- one boundary each, the sixth in the
    second tile) and of a 16-byte piece (bits 16..18 of `expect`), rows that end in a complete character in front of rows
    that begin with one, and a tile that ends in one.  The route is "tile": a spurious malformed flag sends the column
    row-wise"""
    combos = [(ch.encode(), d) for ch in "é€😀" for d in range(1, len(ch.encode()))]
    rows, cur = [], 0
    for k, (ch, d) in enumerate(combos[:5]):
        at = 1024 * (k + 1) - d  # the staged position of a lead byte of this row
        fill = (at - cur) % len(ch)
        rows.append(b"p" * fill + ch * ((at - cur - fill) // len(ch) + 2) + b" " + ch)
        cur += len(rows[-1])
    rows += [ch.encode() for ch in "é€😀"] * 4
    rows += [b"ab", b"cd", b"", b"ef gh", b" ij", b"kl "]  # tokens that open a row behind a kept byte / a delimiter
    rows += ["é".encode()] * (64 - len(rows))               # row 63 ends the first tile in a character, row 64 opens the next with one
    g0 = sum(len(r) for r in rows)
    ch, d = combos[5]
    fill = (1024 - d - (g0 & 15)) % len(ch)
    rows += [b"p" * fill + ch * ((1024 - d - (g0 & 15) - fill) // len(ch) + 2) + b" z", "é".encode(), b"q r"]
    c = Column(rows)
    p = tok_plan(c.offsets())
    assert (p.R, p.route) == (64, "tile") and len(rows) == 67, p
    at = lead_positions(rows)
    for w in (2, 3, 4):
        for d in range(1, w):
            assert any(x == w and pos % 1024 == 1024 - d for x, pos in at), ("chunk row", w, d)
            assert any(x == w and pos % 16 == 16 - d for x, pos in at), ("piece", w, d)
    return c


def col_tok_chunk_rows():
    """32-row tiles of 96-byte rows without a delimiter: bytes 1023 | 1024 and 2047 | 2048 of a tile lie inside rows 10 and
    21 -- kept on both sides, so carry_keep decides that no token opens there -- and every row opens a token directly behind
    the kept last byte of the row in front (`rs`); the second tile has delimiters AT bytes 1023 and 2048"""
    rows = [bytes([97 + i % 26]) * 96 for i in range(32 * 2 + 3)]
    r = bytearray(rows[32 + 10])
    r[1023 - 960] = 32
    rows[32 + 10] = bytes(r)
    r = bytearray(rows[32 + 21])
    r[2048 - 2016] = 32
    rows[32 + 21] = bytes(r)
    c = Column(rows)
    p = tok_plan(c.offsets())
    assert (p.R, p.route) == (32, "tile"), p
    return c


def col_tok_no_tokens(whole=True):
    """rows of delimiters, empty and null rows: a whole column (ntok == 0) or one 64-row tile among tiles with tokens"""
    blank = [(b"  ", b"", None, b" \t\n ", b" ")[i % 5] for i in range(64)]
    rows = blank + blank[:9] if whole else [b"a b"] * 64 + blank + [b"c", b" d "] * 20
    c = Column(rows)
    assert tok_plan(c.offsets()).R == 64
    return c


# (the issue's pool without FF and F8: with three of fifteen bytes announcing four, the reference read behind 34% of the
# malformed rows of 0 to 11 bytes -- a token behind such a byte begins behind the row; the cap is a third)
MALFORMED_POOL = list(b"ab c\t") + [0x00, 0xC3, 0xA9, 0xE2, 0x82, 0x80, 0x1F, 0xF0]


def col_tok_malformed(rows=5000, seed=1, hi=12):
    """rows of 0 to 11 arbitrary bytes"""
    rng = np.random.default_rng(seed)
    pool = np.array(MALFORMED_POOL, dtype=np.uint8)
    return Column([pool[rng.integers(0, len(pool), int(n))].tobytes() for n in rng.integers(0, hi, rows)])


def malformed_edge_columns():
    """one malformation each, at an edge of k_tok_tile's UTF-8 check; every column must go row-wise.  name -> Column"""
    e, eu = "é".encode(), "€".encode()
    out = {}
    base = [b"ab cd"] * 70
    for name, row in (("piece-lead-15", b"x" * 15 + e[:1] + b"y z"), ("piece-lead-14", b"x" * 14 + eu[:2] + b"y"),
                      ("piece-lead3-15", b"x" * 15 + eu[:1] + eu[1:2] + b"y"), ("piece-cont-0", b"x" * 16 + e[1:] + b" z"),
                      ("piece-lead4-13", b"x" * 13 + b"\xf0\x9f\x98" + b" y")):
        rows = list(base)
        rows[0] = row
        out[name] = Column(rows)
    rows = [b"x" * 16] * 70  # a tile is 1024 bytes: row 63 ends at byte 1023
    rows[63] = b"x" * 15 + e[:1]
    out["tile-end-lead"] = Column(list(rows))
    rows[64] = e[1:] + b"x" * 15  # C3 | A9 across two rows and two tiles: well-formed as a stream of bytes, not per row
    out["tile-end-split-char"] = Column(list(rows))
    rows = [b"ab", b"c" + e[:1], e[1:] + b"d", b"ef"] + [b"g h"] * 66
    out["row-start-split-char"] = Column(rows)
    rows = [b"ab cd"] * 70
    rows[69] = b"ab" + eu[:2]
    out["column-end-lead"] = Column(rows)
    rows = [b"w" * 96] * 40  # 32-row tiles: byte 1023 is byte 63 of row 10
    rows[10] = b"w" * 63 + e[:1] + b"w" * 32
    out["chunk-row-lead-63"] = Column(rows)
    seg = col_tok_segs().rows
    seg[1] = seg[1][:-1] + e[:1]  # the last byte of segment 0 announces a byte that row 3 does not bring
    out["segment-end-lead"] = Column(seg)
    for c in out.values():
        assert sum(not well_formed(r) for r in c.rows if r is not None) in (1, 2)
    return out


TokCase = collections.namedtuple("TokCase", "name build delims route outliers")


def tok_cases():
    """name, the column's builder, the delimiter sets, the route the table fixes for whitespace and ASCII sets of up to four
    (ROWS_SETS always go "rows"), CS_NO_OUTLIER_TILES"""
    cases = []
    for shape in SHAPES:
        cases.append(TokCase("shape-" + shape, lambda shape=shape: col_tok_shape(shape), SETS + ["_- "], "tile", True))
    cases.append(TokCase("segs", col_tok_segs, [None, " ", " ."], "tile-segs", True))
    cases.append(TokCase("segs-no-outlier-tiles", col_tok_segs, [None, " "], "rows", False))
    cases.append(TokCase("utf8-edges", col_tok_utf8_edges, [None, " ", "p "], "tile", True))
    cases.append(TokCase("chunk-rows", col_tok_chunk_rows, [None, " ", "_-"], "tile", True))
    cases.append(TokCase("no-token-column", col_tok_no_tokens, [None, " ", " \t\n"], "tile", True))
    cases.append(TokCase("no-token-tile", lambda: col_tok_no_tokens(False), [None, " "], "tile", True))
    for name, c in malformed_edge_columns().items():
        cases.append(TokCase("malformed-" + name, lambda c=c: c, [None, " "], "rows", True))
    # the route of arbitrary bytes is what the fix makes it: the kernel's check hands the column to the row-wise walk
    cases.append(TokCase("malformed-pool", col_tok_malformed, [None, " ", " .", "_-"], "rows", True))
    return cases


# ---- ngrams: the columns ---------------------------------------------------------------------------------------------------------
def _token(i, size):
    return (b"%d." % i + b"abcdefghijklmnopqrstuvwxyz" * (size // 26 + 1))[:size] if size > 2 else b"xyz"[:size]


def toks_lengths(count, seed=3):
    """tokens of 1 .. 33 bytes, 15, 16 and 17 (or_bytes hands over to lds_copy beyond 16) among them, at every source and
    destination alignment: the lengths are drawn, so runs of every residue mod 4 follow one another"""
    rng = np.random.default_rng(seed + count)
    sizes = rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33], count)
    return [_token(i, int(s)) for i, s in enumerate(sizes)]


def toks_sized(count, size):
    rows = [_token(i, size) for i in range(count)]
    assert {len(r) for r in rows} == {size}
    return rows


NgCase = collections.namedtuple("NgCase", "name build n sep m_first route")


def ng_cases():
    cases = []

    def add(name, build, n, sep, m_first=8, route=None):
        cases.append(NgCase(name, build, n, sep, m_first, route))

    for sepn in range(0, 10):  # 9: row-wise
        add("sep-%d" % sepn, lambda: toks_lengths(64 * 2 + 5), 3, b"123456789"[:sepn], route=None if sepn <= 8 else "rows")
    for n in range(1, 10):     # 1 and 9: row-wise
        add("n-%d" % n, lambda: toks_lengths(64 * 2 + 5), n, b"_", route=None if 2 <= n <= 8 else "rows")
    for n in (2, 8):
        add("rows-eq-n-%d" % n, lambda n=n: toks_lengths(n), n, b"_", route="rows")
        add("rows-eq-n+1-%d" % n, lambda n=n: toks_lengths(n + 1), n, b"-")
    for size in (15, 16, 17):
        add("len-%d" % size, lambda size=size: toks_sized(200, size), 2, b"_")
        add("len-%d-sep3" % size, lambda size=size: [b"a", b"bc", b"def"] + toks_sized(200, size), 3, b"+-+")
    for m in (8, 4, 2, 1):
        for extra in (1, 63, 64, 65):
            add("m%d-last-%d" % (m, extra), lambda m=m, extra=extra: toks_sized(64 * m + extra + 1, 3), 2, b"", m_first=m,
                route="tile-m%d" % m)
    # 40-byte tokens: 512 bigrams are 41 KB of output, beyond 12 KB - 64 at M = 8 and 4; 2 fits
    add("forced-m2", lambda: toks_sized(700, 40), 2, b"_", route="tile-m2")
    add("forced-m1", lambda: toks_sized(300, 90), 2, b"_", route="tile-m1")
    add("input-bound-m1", toks_input_bound, 2, b"", route="tile-m1")
    add("fits-no-m", lambda: toks_sized(200, 40) + [b"L" * 7000] + toks_sized(100, 40), 2, b"_", route="rows")
    for where, at in (("first", 0), ("middle", 100), ("last", 199)):
        for hole in (None, b""):
            def build(at=at, hole=hole):
                t = toks_lengths(200)
                t[at] = hole
                return t
            add("hole-%s-%s" % (where, "null" if hole is None else "empty"), build, 2, b"_", route="rows")
    return cases


def ng_route(case, rows):
    want = ngram_route(rows, case.n, case.sep, case.m_first)
    assert case.route in (None, want), (case.name, case.route, want)
    return want
