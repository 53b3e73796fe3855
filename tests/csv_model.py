"""Python model of from_csv (the reference's createFromCSV, cpp/src/util.cu:42-169), written independently of
custrings_amd/csrc/csv_ops.h and cs_csv.hip, and the g++ harness that runs csv_ops.h itself behind a sequential line finder.
A file is bytes; a column is a list of bytes / None (a null row); a file the loader refuses is None."""
import os
import re
import subprocess

import numpy as np

SORT_LENGTH, SORT_NAME, NULL_IS_EMPTY = 1, 2, 8
LINE_END = re.compile(rb"[\r\n][\x01-\x1f]*")  # a terminator and every control byte behind it (tabs count)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def text_of(data):
    """the bytes the line scan sees: up to the first NUL, and the '\\r' the loader appends (behind the NUL it is never seen)"""
    data = bytes(data)
    cut = data.find(b"\0")
    return data[:cut] if cut >= 0 else data + b"\r"


def line_starts(data, lines=0):
    """positions behind each line end; the header's own start (0) is not recorded; `lines` > 0 keeps lines + 1 of them"""
    starts = [m.end() for m in LINE_END.finditer(text_of(data))]
    return starts[:lines + 1] if lines > 0 else starts


def field_of(span, column, null_is_empty=False):
    """-> (bytes or None, entered quoted mode in the field returned).  span: a row with its line end."""
    m = re.search(rb"[\r\n]", span)
    row = bytearray(span)
    if m:
        row[m.start()] = 0  # the first terminator reads as 0; later ones read raw
    begin, length, col, quoted, was_quoted, i = 0, 0, 0, False, False, 0
    while i < len(row):
        ch = row[i]
        i += 1
        if ch == 0x22:
            if quoted:
                if i < len(row) and row[i] == 0x22:
                    i += 1
                    length += 2  # the pair stays
                else:
                    quoted = False
            elif length == 0:
                quoted = was_quoted = True
                begin += 1
            continue  # (a quote behind content: dropped from the count, not from the span)
        if ch != 0 and (quoted or ch != 0x2C):
            length += 1
            continue
        if col >= column:
            break
        col += 1
        begin, length, quoted, was_quoted = i, 0, False, False
    if length == 0 and not null_is_empty:
        return None, was_quoted
    return bytes(span[begin:begin + length]), was_quoted


def order(rows, flags):
    """ascending, nulls first, equal keys in row order (what sort gives)"""
    if not flags & (SORT_LENGTH | SORT_NAME):
        return list(rows)

    def key(r):
        if r is None:
            return (0,)
        return (1, len(r) if flags & SORT_LENGTH else 0, r if flags & SORT_NAME else b"")

    return sorted(rows, key=key)


def spans_of(data, lines=0):
    text, starts = text_of(data), line_starts(data, lines)
    return [text[a:b] for a, b in zip(starts, starts[1:])]


def from_csv_buffer(data, column, lines=0, flags=0):
    rows = [field_of(s, column, bool(flags & NULL_IS_EMPTY))[0] for s in spans_of(data, lines)]
    return order(rows, flags)


def from_csv(path, column, lines=0, flags=0):
    """None: a file that is missing or shorter than 2 bytes"""
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return None
    return None if len(data) < 2 else from_csv_buffer(data, column, lines, flags)


# ---- generated files -----------------------------------------------------------------------------------------------------------
POOL = np.frombuffer(b'abcXYZ019 .-_;:/' + b'"' * 6 + b"," * 8 + b"\r" * 2 + b"\n" * 3 + b"\t" * 2 + b"\x01\x1f" + bytes([0xC3, 0xA9, 0xE2, 0x82, 0xAC, 0xFF, 0x80]),
                     dtype=np.uint8)


def gen_buffers(nlines, seed, per=400, nul_rate=0.5):
    """files of about `per` lines each over POOL (quotes, commas, both terminators, tabs, other control bytes, bytes >= 0x80),
    about `nlines` lines in all; `nul_rate` of them hold NUL bytes in their last tenth (the text ends at the first)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(max(1, nlines // per)):
        n = per * 14  # (5 terminators among 37 pool bytes, runs merged: about 14 bytes a line)
        buf = POOL[rng.integers(0, len(POOL), size=n)].copy()
        # some well-formed quoted fields among the noise
        for p in rng.integers(0, n - 12, size=per // 4).tolist():
            buf[p:p + 11] = np.frombuffer(b',"q,""x""",', dtype=np.uint8)
        if rng.random() < nul_rate:
            buf[rng.integers(n - n // 10, n, size=3)] = 0
        out.append(buf.tobytes())
    return out


def gen_lines(n, seed, shape="mixed"):
    """one well-formed file of n data lines behind a header: 'log' (a C3-like line, no quotes), 'tweets' (9 columns, the text
    column quoted with "" pairs inside) or 'mixed' (both, empty fields, \\r\\n and blank lines)"""
    rng = np.random.default_rng(seed)
    words = ["GET", "/index.html", "200", "10.0.0.7", "nice to know", "paper is the best", "http://t.co/x", "é€", "", "a,b"]
    rows = [b"h0,h1,h2,h3,h4,h5,h6,h7,h8"]
    picks = rng.integers(0, len(words), size=(n, 9))
    ends = rng.integers(0, 4, size=n)
    for r in range(n):
        kind = shape if shape != "mixed" else ("log", "tweets")[r & 1]
        f = [words[k] for k in picks[r]]
        if kind == "tweets":
            f = [w if "," not in w else '"%s"' % w for w in f]
            f[7] = '"%s said ""%s"", twice"' % (f[0], f[1].strip('"'))
        else:
            f = [w.replace(",", ";") for w in f[:5]]
        end = b"\n" if shape != "mixed" else (b"\n", b"\r\n", b"\n\n", b"\n\t")[ends[r]]
        rows.append(",".join(f).encode() + end)
    rows[0] += b"\n"
    return b"".join(rows)


# ---- the harness: csv_ops.h built with g++ behind the reference's sequential line scan ----------------------------------------
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "csv_ops.h"
template <class T> static std::vector<T> slurp(const char* path) {
  std::vector<T> v;
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
// harness COLUMN LINES FLAGS BYTES SIZES OUT
// BYTES: the files back to back, SIZES: int64 bytes of each.  OUT, per file: int64 rows, then per row int64 begin (in the
// file; -1 null) and int64 length.  Every file is scanned in a buffer of exactly its bytes, the '\r' and the NUL the loader
// appends; every row is walked in a buffer of exactly its span (a read past it is the sanitizer's).
int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const unsigned column = (unsigned)atoi(argv[1]), lines = (unsigned)atoi(argv[2]), flags = (unsigned)atoi(argv[3]);
  std::vector<uint8_t> bytes = slurp<uint8_t>(argv[4]);
  std::vector<int64_t> sizes = slurp<int64_t>(argv[5]), out;
  size_t at = 0;
  for (size_t k = 0; k < sizes.size(); ++k) {
    const size_t n = (size_t)sizes[k];
    uint8_t* text = new uint8_t[n + 2];
    if (n) memcpy(text, bytes.data() + at, n);
    at += n;
    text[n] = '\r';
    text[n + 1] = 0;
    std::vector<size_t> starts;  // util.cu:67-84, nothing written into the text
    for (size_t p = 0; text[p];) {
      if (!cscsv::is_terminator(text[p])) { ++p; continue; }
      do ++p; while (cscsv::is_control(text[p]));
      starts.push_back(p);
      if (lines && starts.size() > lines) break;
    }
    if (!lines) {  // the same starts from the 16-byte pieces the kernels walk (exit 5), each piece's masks byte by byte (exit 6)
      const size_t z = strlen((const char*)text);
      std::vector<size_t> by_piece;
      int state = 0;
      for (size_t p0 = 0; p0 <= z; p0 += cscsv::kPieceBytes) {
        uint8_t piece[cscsv::kPieceBytes] = {0};
        memcpy(piece, text + p0, n + 2 - p0 < sizeof(piece) ? n + 2 - p0 : sizeof(piece));
        uint32_t w[4];
        memcpy(w, piece, sizeof(piece));
        const cscsv::Piece pc = cscsv::classify(w);
        for (int i = 0; i < cscsv::kPieceBytes; ++i)
          if (((pc.control >> i) & 1) != (unsigned)cscsv::is_control(piece[i]) || ((pc.terminator >> i) & 1) != (unsigned)cscsv::is_terminator(piece[i]) ||
              ((pc.nul >> i) & 1) != (unsigned)(piece[i] == 0))
            return 6;
        int next;
        const uint32_t m = cscsv::piece_starts(pc, state, next);
        state = next;
        for (int i = 0; i < cscsv::kPieceBytes; ++i)
          if (((m >> i) & 1) && p0 + i <= z) by_piece.push_back(p0 + i);
      }
      if (by_piece != starts) return 5;
    }
    const size_t rows = starts.empty() ? 0 : starts.size() - 1;
    out.push_back((int64_t)rows);
    for (size_t r = 0; r < rows; ++r) {
      const size_t span = starts[r + 1] - starts[r];
      uint8_t* row = new uint8_t[span];
      memcpy(row, text + starts[r], span);
      const cscsv::Field f = cscsv::locate_field(row, (int)span, column, (flags & cscsv::kNullIsEmpty) != 0);
      delete[] row;
      if (!f.is_null() && (f.begin < 0 || f.length < 0 || (size_t)f.begin + (size_t)f.length > span)) return 3;
      out.push_back(f.is_null() ? -1 : (int64_t)(starts[r] + f.begin));
      out.push_back(f.is_null() ? 0 : f.length);
    }
    delete[] text;
  }
  FILE* f = fopen(argv[6], "wb");
  fwrite(out.data(), 8, out.size(), f);
  fclose(f);
  return 0;
}
"""


class Harness:
    """csv_ops.h built with g++ and the address / undefined-behaviour sanitizers into `workdir`; it runs as a child process"""

    def __init__(self, workdir, root):
        self.dir = workdir
        src = os.path.join(workdir, "csv_harness.cpp")
        self.exe = os.path.join(workdir, "csv_harness")
        open(src, "w").write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-I",
                        os.path.join(root, "custrings_amd", "csrc"), src, "-o", self.exe], check=True)

    def run(self, buffers, column, lines=0, flags=0):
        """files -> one column each (unsorted: the harness stops at the (begin, length) pairs)"""
        bpath, spath, out = (os.path.join(self.dir, n) for n in ("bytes.bin", "sizes.bin", "out.bin"))
        with open(bpath, "wb") as f:
            f.write(b"".join(buffers))
        np.array([len(x) for x in buffers], dtype=np.int64).tofile(spath)
        done = subprocess.run([self.exe, str(column), str(lines), str(flags), bpath, spath, out], timeout=900, capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
        data = np.fromfile(out, dtype=np.int64).tolist()
        res, k = [], 0
        for buf in buffers:
            text = bytes(buf) + b"\r"
            rows = data[k]
            k += 1
            col = []
            for _ in range(rows):
                begin, length = data[k], data[k + 1]
                k += 2
                col.append(None if begin < 0 else text[begin:begin + length])
            res.append(col)
        assert k == len(data)
        return res
