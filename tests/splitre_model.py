"""The model of split_re / rsplit_re (custrings_amd/csrc/splitre_ops.h states the definition).

A row's matches x[0..m-1] and the tokens t[0..m] between them come from three calls on engines.OracleEngine: findall,
replace_re(pat, SEP, -1) and split(SEP), SEP being a byte the rows do not hold.  With s = m (no limit) or min(m, limit)
cuts, split_re gives t[:s] and then t[s] + x[s] + t[s + 1] + ... + t[m]; rsplit_re is the mirror image.  Nothing here
finds a match itself.

Harness: splitre_ops.h (the text the kernel compiles) built with g++, fed the model's match spans."""
import os
import subprocess

import engines

ROOT = engines.ROOT
SEP = "\x01"

_orc = None


def oracle():
    global _orc
    if _orc is None:
        _orc = engines.OracleEngine()
    return _orc


_pieces = {}


def pieces(rows, pat):
    """-> per row None (a null row) or (tokens t[0..m], matches x[0..m-1]); computed once per (rows, pattern)"""
    key = (tuple(rows), pat)
    if key not in _pieces:
        _pieces[key] = _pieces_of(rows, pat)
    return _pieces[key]


def _pieces_of(rows, pat):
    assert not any(r is not None and SEP in r for r in rows)
    if not rows:
        return []
    orc = oracle()
    found = orc.findall(rows, pat)
    toks = orc.split(orc.replace_re(rows, pat, SEP, -1), SEP)
    out = []
    for i, row in enumerate(rows):
        if row is None:
            out.append(None)
            continue
        x = [c[i] for c in found if c[i] is not None]
        t = [c[i] for c in toks if c[i] is not None] or [""]
        assert len(t) == len(x) + 1 and "".join(a + b for a, b in zip(t, x + [""])) == row, (row, pat, t, x)
        out.append((t, x))
    return out


def cut(t, x, limit, reverse):
    """one row's tokens"""
    m = len(x)
    s = m if limit <= 0 else min(m, limit)
    if not reverse:
        return t[:s] + [t[s] + "".join(a + b for a, b in zip(x[s:], t[s + 1:]))]
    return ["".join(a + b for a, b in zip(t[:m - s], x[:m - s])) + t[m - s]] + t[m - s + 1:]


def records(rows, pat, limit=-1, reverse=False):
    """-> per row its tokens; a null row: None"""
    return [None if p is None else cut(p[0], p[1], limit, reverse) for p in pieces(rows, pat)]


def columns(rows, pat, limit=-1, reverse=False):
    """the column-major result: column k = every row's token k, None from its token count on.  No rows, or null rows
    only: one column of nulls, as split answers."""
    recs = records(rows, pat, limit, reverse)
    ncols = max([len(r) for r in recs if r is not None], default=1)
    return [[r[k] if r is not None and k < len(r) else None for r in recs] for k in range(ncols)]


def match_spans(rows, pat):
    """-> per row None or its matches as (begin, length) in bytes"""
    out = []
    for p in pieces(rows, pat):
        if p is None:
            out.append(None)
            continue
        at, spans = 0, []
        for tok, hit in zip(p[0], p[1]):
            at += len(tok.encode("utf8"))
            spans.append((at, len(hit.encode("utf8"))))
            at += spans[-1][1]
        out.append(spans)
    return out


HARNESS = r"""
#include <stdio.h>
#include <vector>
#include "splitre_ops.h"
// in: maxsplit reverse ncols nrows, then per row: n m and m pairs (begin, length).  out: per row and column "begin length", or "-1 -1"
int main(int argc, char** argv) {
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  int maxsplit, reverse, ncols, nrows;
  if (!in || !out || fscanf(in, "%d %d %d %d", &maxsplit, &reverse, &ncols, &nrows) != 4) return 1;
  for (int r = 0; r < nrows; ++r) {
    int n, m;
    if (fscanf(in, "%d %d", &n, &m) != 2) return 1;
    std::vector<int> mb(m), ml(m);
    for (int j = 0; j < m; ++j)
      if (fscanf(in, "%d %d", &mb[j], &ml[j]) != 2) return 1;
    const int s = cssre::cuts(m, maxsplit), c0 = cssre::first_cut(m, s, reverse != 0);
    cssre::Walk w;
    for (int k = 0; k < ncols; ++k) {
      int tb = 0, tl = 0;
      const bool cutk = k < s;
      const bool has = cssre::token_span(w, k, s, n, cutk ? mb[c0 + k] : n, cutk ? ml[c0 + k] : 0, tb, tl);
      fprintf(out, "%d %d\n", has ? tb : -1, has ? tl : -1);
    }
  }
  fclose(out);
  return 0;
}
"""


class Harness:
    """splitre_ops.h built with g++ into `workdir`"""

    def __init__(self, workdir, root=ROOT):
        self.dir = workdir
        src = os.path.join(workdir, "splitre_harness.cpp")
        self.exe = os.path.join(workdir, "splitre_harness")
        open(src, "w").write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "custrings_amd", "csrc"), src, "-o", self.exe], check=True)

    def records(self, rows, spans, limit, reverse, ncols):
        """valid rows (str) and their match spans -> per row its tokens, cut from the row's bytes by token_span"""
        inp, outp = os.path.join(self.dir, "in.txt"), os.path.join(self.dir, "out.txt")
        with open(inp, "w") as f:
            f.write("%d %d %d %d\n" % (limit, int(reverse), ncols, len(rows)))
            for row, sp in zip(rows, spans):
                f.write("%d %d %s\n" % (len(row.encode("utf8")), len(sp), " ".join("%d %d" % p for p in sp)))
        subprocess.run([self.exe, inp, outp], check=True, timeout=120)
        vals = [tuple(int(v) for v in line.split()) for line in open(outp)]
        out = []
        for i, row in enumerate(rows):
            raw = row.encode("utf8")
            out.append([raw[b:b + n].decode("utf8") for b, n in vals[i * ncols:(i + 1) * ncols] if b >= 0])
        return out
