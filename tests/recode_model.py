"""Python model of url_encode / url_decode / translate / fillna (custrings_amd/csrc/recode_ops.h), written independently of
it, and the g++ harness that runs the header itself.  Rows are bytes (None: a null row); the str entry points are for the
golden cases."""
import os
import subprocess
import urllib.parse

import numpy as np

UNRESERVED = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz._~-"
OPS = {"url_encode": 0, "url_decode": 1, "translate": 2}


# ---- the model ------------------------------------------------------------------------------------------------------------------
def encode_row(row):
    """urllib's quote with no safe characters: Python's always-safe set is the reference's unreserved set"""
    return urllib.parse.quote(row, safe="").encode("ascii")


def hex_value(c):
    if 48 <= c <= 57:
        return c - 48
    if 65 <= c <= 90:  # all of A-Z
        return c - 55
    if 97 <= c <= 122:
        return c - 87
    return 0


def decode_row(row):
    out, i, n = bytearray(), 0, len(row)
    while i < n:
        if row[i] == 0x25 and i + 2 < n:  # '%' with at least two bytes AFTER it
            out.append(((hex_value(row[i + 1]) * 16) % 256 + hex_value(row[i + 2])) % 256)
            i += 3
        else:
            out.append(row[i])
            i += 1
    return bytes(out)


def table_of(pairs):
    """the caller's (key, target) pairs as a dict for str.translate: the last pair of a key wins, target 0 deletes"""
    return {int(k): (None if not v else int(v)) for k, v in pairs}


def _char_at(row, i):
    """-> (bytes the character takes, its str or None for a malformed sequence): by lead byte, cut at the row's end"""
    b = row[i]
    if b < 0x80:
        return 1, chr(b)
    if b & 0xC0 == 0x80:
        return 1, None
    w = 2 if b < 0xE0 else 3 if b < 0xF0 else 4
    if i + w > len(row):
        return len(row) - i, None
    try:
        return w, row[i:i + w].decode("utf-8")  # (strict: over-long forms, encoded surrogates and bytes >= 0xF8 do not decode)
    except UnicodeDecodeError:
        return w, None


def translate_row(row, pairs):
    table = table_of(pairs)
    try:
        return row.decode("utf-8").translate(table).encode("utf-8")
    except UnicodeDecodeError:
        pass
    out, i = bytearray(), 0
    while i < len(row):
        w, ch = _char_at(row, i)
        if ch is None or ord(ch) not in table:
            out += row[i:i + w]
        elif table[ord(ch)] is not None:
            out += chr(table[ord(ch)]).encode("utf-8", "surrogatepass")
        i += w
    return bytes(out)


def apply_column(op, rows, pairs=None):
    f = {"url_encode": encode_row, "url_decode": decode_row, "translate": lambda r: translate_row(r, pairs)}[op]
    return [None if r is None else f(r) for r in rows]


def fillna_column(rows, repl):
    """repl: bytes, or a list of bytes / None of the same length"""
    if isinstance(repl, (bytes, bytearray)):
        return [repl if r is None else r for r in rows]
    assert len(repl) == len(rows)
    return [repl[i] if r is None else r for i, r in enumerate(rows)]


def apply_case(case):
    """a golden case (str rows) through the model -> str rows"""
    rows = [None if r is None else r.encode() for r in case["input"]]
    op = case["op"]
    if op == "fillna":
        a = case["args"]
        got = fillna_column(rows, a["str"].encode() if "str" in a else [None if r is None else r.encode() for r in a["column"]])
    elif op in ("index", "rindex"):
        sub = case["args"][0]
        return [None if r is None else (r.find(sub) if op == "index" else r.rfind(sub)) for r in case["input"]]
    else:
        got = apply_column(op, rows, case["args"])
    return [None if r is None else r.decode() for r in got]


# ---- generated rows ------------------------------------------------------------------------------------------------------------
ALPHABET = ["a", "b", "Z", "0", "7", "-", "_", ".", "~", " ", "/", "+", "%", "%", "4", "1", "f", "C", "z", "\t", "\x00", "é", "ñ", "ß", "€", "中",
            "😀", "\x7f"]


def gen_rows(n, seed, maxlen=24, null_rate=0.05):
    """valid UTF-8 rows over ALPHABET (NUL bytes, runs of '%', 1 - 4 byte characters)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, size=n)
    lens[rng.random(n) < 0.05] = 0
    picks = rng.integers(0, len(ALPHABET), size=int(lens.sum()))
    nulls = rng.random(n) < null_rate
    enc = [a.encode() for a in ALPHABET]
    rows, k = [], 0
    for i in range(n):
        L = int(lens[i])
        rows.append(None if nulls[i] else b"".join(enc[j] for j in picks[k:k + L]))
        k += L
    return rows


def gen_byte_rows(n, seed, maxlen=12):
    """rows of arbitrary bytes, weighted towards '%', hex digits and UTF-8 lead / continuation bytes"""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.arange(256), np.full(40, 0x25), np.frombuffer(b"0123456789abcdefABCDEFzZ", dtype=np.uint8),
                           np.array([0xC3, 0xA9, 0xE2, 0x82, 0xAC, 0xF0, 0x9F, 0x98, 0x80, 0xC0, 0x80, 0xF8, 0xFF, 0xED, 0xA0] * 3)]).astype(np.uint8)
    lens = rng.integers(0, maxlen + 1, size=n)
    data = pool[rng.integers(0, len(pool), size=int(lens.sum()))].tobytes()
    rows, k = [], 0
    for L in lens.tolist():
        rows.append(data[k:k + L])
        k += L
    return rows


def percent_tail_rows():
    """'%' at each of the last three positions, runs of '%', the issue's examples"""
    rows = [b"%41", b"%4", b"a%", b"%%41", b"%zz", b"%", b"%%", b"%%%", b"%%%%", b"ab%", b"ab%4", b"ab%41", b"%4%41", b"%e2%82%ac", b"%C3%A9",
            b"100%", b"%%%41%", b"%25%2541", b"\x00%00\x00", b""]
    for body in (b"x", b"xy%20", "é".encode()):
        for tail in (b"%", b"%a", b"%ab", b"%%", b"%%a", b"%%ab"):
            rows.append(body + tail)
    return rows


def to_arrow(rows):
    """-> chars uint8, offsets int64 (rows + 1), nulls uint8 (1 = null)"""
    lens = np.array([0 if r is None else len(r) for r in rows], dtype=np.int64)
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = np.frombuffer(b"".join(r for r in rows if r is not None), dtype=np.uint8)
    nulls = np.array([r is None for r in rows], dtype=np.uint8)
    return chars, offs, nulls


# ---- the harness: recode_ops.h built with g++ -----------------------------------------------------------------------------------
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "recode_ops.h"
template <class T> static std::vector<T> slurp(const char* path) {
  std::vector<T> v;
  if (!strcmp(path, "-")) return v;
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize(n / sizeof(T) + 1);
  if (n && fread(v.data(), 1, n, f) != (size_t)n) exit(2);
  v.resize(n / sizeof(T));
  return v;
}
// harness OP FROM TO CHARS OFFS NULLS OUT
// OUT: int64 length per row (-1 null), then the rows' bytes.  Every row is read from a buffer of exactly its bytes and
// written into one of exactly the size the size function gave (the sanitizer sees a byte too many); a byte too few: exit 3.
int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int op = atoi(argv[1]);
  std::vector<uint32_t> from = slurp<uint32_t>(argv[2]), to = slurp<uint32_t>(argv[3]);
  csrecode::HostTable h;
  if (!csrecode::make_table(from.data(), to.data(), (int)from.size(), h)) return 4;
  csrecode::Table t{h.ascii, h.keys.data(), h.vals.data(), (int)h.keys.size()};
  const csrecode::SafeMask safe = csrecode::url_safe_mask();
  std::vector<uint8_t> chars = slurp<uint8_t>(argv[4]), nulls = slurp<uint8_t>(argv[6]);
  std::vector<int64_t> offs = slurp<int64_t>(argv[5]);
  const size_t rows = offs.size() - 1;
  std::vector<int64_t> lens(rows);
  std::vector<uint8_t> out;
  for (size_t r = 0; r < rows; ++r) {
    if (nulls[r]) { lens[r] = -1; continue; }
    const int n = (int)(offs[r + 1] - offs[r]);
    uint8_t* p = new uint8_t[n];  // (exactly n bytes: a read past the row is the sanitizer's)
    if (n) memcpy(p, chars.data() + offs[r], n);
    const int64_t sz = op == 0 ? csrecode::encode_size(safe, p, n) : op == 1 ? csrecode::decode_size(p, n) : csrecode::translate_size(t, p, n);
    // written twice over different fills: a byte the write leaves out differs between the two
    uint8_t* o[2] = {new uint8_t[sz], new uint8_t[sz]};
    for (int k = 0; k < 2; ++k) {
      memset(o[k], k ? 0x54 : 0xAB, (size_t)sz);
      if (op == 0) csrecode::encode_write(safe, p, n, o[k]);
      else if (op == 1) csrecode::decode_write(p, n, o[k]);
      else csrecode::translate_write(t, p, n, o[k]);
    }
    if (memcmp(o[0], o[1], (size_t)sz) != 0) return 3;
    out.insert(out.end(), o[0], o[0] + sz);
    delete[] p;
    delete[] o[0];
    delete[] o[1];
    lens[r] = sz;
  }
  FILE* f = fopen(argv[7], "wb");
  fwrite(lens.data(), 8, rows, f);
  fwrite(out.data(), 1, out.size(), f);
  fclose(f);
  return 0;
}
"""


class Harness:
    """recode_ops.h built with g++ and the address / undefined-behaviour sanitizers into `workdir`; it runs as a child process"""

    def __init__(self, workdir, root):
        self.dir = workdir
        src = os.path.join(workdir, "recode_harness.cpp")
        self.exe = os.path.join(workdir, "recode_harness")
        open(src, "w").write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-I",
                        os.path.join(root, "custrings_amd", "csrc"), src, "-o", self.exe], check=True)

    def _file(self, name, data):
        if data is None:
            return "-"
        p = os.path.join(self.dir, name)
        np.ascontiguousarray(data).tofile(p)
        return p

    def run(self, op, rows, pairs=None):
        """rows of bytes / None -> rows of bytes / None"""
        chars, offs, nulls = to_arrow(rows)
        pairs = pairs or []
        args = [str(OPS[op]), self._file("from.bin", np.array([p[0] for p in pairs], dtype=np.uint32) if pairs else None),
                self._file("to.bin", np.array([p[1] for p in pairs], dtype=np.uint32) if pairs else None),
                self._file("c.bin", chars), self._file("o.bin", offs), self._file("n.bin", nulls)]
        out = os.path.join(self.dir, "out.bin")
        done = subprocess.run([self.exe] + args + [out], timeout=900, capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
        data = np.fromfile(out, dtype=np.uint8)
        n = len(offs) - 1
        lens = data[:8 * n].view(np.int64)
        body = data[8 * n:].tobytes()
        res, k = [], 0
        for L in lens.tolist():
            if L < 0:
                res.append(None)
            else:
                res.append(body[k:k + L])
                k += L
        assert k == len(body)
        return res
