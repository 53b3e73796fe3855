#!/usr/bin/env python3
"""Per-operation throughput of every SURVEY section-8(a) row on the synthetic configs of
BASELINE.json (C2-C5), one GPU, inputs resident in HBM.  Secondary to bench.py (which is the
headline metric): this prints one JSON line per op with wall time per call (device
synchronised), input GB/s and the fraction of the 8 TB/s HBM roofline over the op's
ALGORITHMIC bytes (SURVEY.md 8d formulas).  Usage: python tools/bench_ops.py [--scale 1.0]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime per process)

from custrings_amd import _lib, nvcategory, nvstrings, nvtext  # noqa: E402

L = _lib.lib
_lib.ensure_init(0)
SEED = 20240607
IPV4 = r"\d+\.\d+\.\d+\.\d+"
IPV4B = r"\b\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}\b"
GTEST = r"(\bin\b)|(\ba\b)|(\bthe\b)"


def synth(kind, rows, param=0):
    out = C.c_void_p()
    _lib.check(L.cs_synth_column(kind, 0, rows, SEED, param, None, C.byref(out)))
    return nvstrings.nvstrings(out.value)


def nbytes(col):
    return int(L.cs_column_nbytes(col.m_cptr))


def col_ov(col):
    """offset + validity bytes per row of an output column, at the offset width it was actually written with (bench.py's rule)"""
    return int(L.cs_column_offset_width(col.m_cptr)) + 0.125


def timed(fn, reps=3):
    fn()  # warm-up (allocator cache, kernel load)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
        del r
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def report(config, op, rows, in_bytes, alg_bytes, dt):
    print(json.dumps({"config": config, "op": op, "rows": rows, "ms": round(dt * 1e3, 3),
                      "input_GBps": round(in_bytes / dt / 1e9, 1), "alg_bytes_per_row": round(alg_bytes / rows, 1),
                      "alg_GBps": round(alg_bytes / dt / 1e9, 1), "frac_of_8TBps": round(alg_bytes / dt / 8e12, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="row-count multiplier (1.0 = BASELINE.json single-GPU sizes)")
    ap.add_argument("--only", default="C2,C3,C4,C5", help="comma-separated configs to run (CONV: the conversion ops, TS: the timestamp ones, PAD: substring / padding / wrapping, CHR: character types and swapcase / capitalize / title, TXT: the NVText matches, edit distance, stemmer measure and scatter_count, URL: url_encode / url_decode / translate / fillna, NUM: the numeric categories -- from_numbers, to_numbers, merge_and_remap -- beside two yardsticks, CSV: from_csv -- the line-start kernels, the field locator and the whole call, STATS: compute_statistics / get_info -- the fused pass beside the separate ops, the histogram layouts, the whole call, MINHASH: minhash on short and long rows at nperm 1 / 64 / 256 and the band keys, SPLITRE: split_re at three patterns with its steps' kernel times beside split and findall, WP: WordPiece tokenize and encode on short and long rows under a 30 000-entry and a 300-entry vocabulary)")
    a = ap.parse_args()
    only = set(a.only.split(","))
    ov = 8.125  # native offset + validity bytes per row

    if "C2" in only:
        run_c2(a, ov)
    if "C3" in only:
        run_c3(a, ov)
    if "C4" in only:
        run_c4(a, ov)
    if "C5" in only:
        run_c5(a, ov)
    if "CONV" in only:
        run_conv(a, ov)
    if "TS" in only:
        run_ts(a)
    if "PAD" in only:
        run_pad(a)
    if "CHR" in only:
        run_chr(a)
    if "TXT" in only:
        run_txt(a)
    if "URL" in only:
        run_url(a)
    if "NUM" in only:
        run_num(a)
    if "CSV" in only:
        run_csv(a)
    if "STATS" in only:
        run_stats(a)
    if "MINHASH" in only:
        run_minhash(a)
    if "SPLITRE" in only:
        run_splitre(a)
    if "WP" in only:
        run_wordpiece(a)


def run_splitre(a):
    """split_re (cs_split_re) on the C3 and C5 columns at 2M rows (x --scale): the whole call at ' ', '\\s+' and
    ' - | \\[|\\] ', the steps' kernel times from the profiling hooks in a run of their own (count scan, span scan, token
    spans, writers) and k_token_spans' share; beside them two yardsticks on the same column -- the literal split(' ') and
    findall('[^ ]+'), the same scan and writers at a width found by a provisional pass."""
    from custrings_amd import splitre

    rows = int(2_000_000 * a.scale)
    kernels = (b"k_count_re", b"k_findall_spans", b"k_token_spans", b"k_extract_write")
    for name, kind in (("C3", 3), ("C5", 5)):
        col = synth(kind, rows)
        n, nb = col.size(), nbytes(col)
        calls = [("split(' ')", lambda: col.split(" ")), ("findall('[^ ]+')", lambda: col.findall("[^ ]+"))]
        calls += [("split_re(%r)" % p, (lambda p: lambda: splitre.split_re(col, p))(p)) for p in (" ", r"\s+", r" - | \[|\] ")]
        for op, fn in calls:
            ncols = len(fn())
            dt = timed(fn, reps=5)
            line = {"config": "SPLITRE " + name, "op": op, "rows": n, "bytes": nb, "columns": ncols, "ms": round(dt * 1e3, 3),
                    "input_GBps": round((nb + 8.125 * n) / dt / 1e9, 1)}
            if op.startswith("split_re"):
                L.cs_prof_reset()
                L.cs_prof_enable(1)
                reps = 3
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                L.cs_prof_enable(0)
                for kern in kernels:
                    ms, k = C.c_double(), C.c_int64()
                    L.cs_prof_get(kern, C.byref(ms), C.byref(k))
                    line[kern.decode() + "_ms"] = round(ms.value / reps, 3)
                line["token_spans_share"] = round(line["k_token_spans_ms"] / (dt * 1e3), 4)
            print(json.dumps(line), flush=True)
        del col


def run_wordpiece(a):
    """WordPiece (cs_wordpiece_*): tokenize (count + write, into device memory) and encode at max_length 128 with cls / sep, with
    punct, on the C3 log-line column and the C5 column at 2M rows (x --scale) and a generated column of 20 000 rows of ~4 KB,
    under a generated vocabulary of 30 000 entries and the 300-entry one of the tests -- the whole call's ms, ids per second,
    the share of unk among them, the form that ran, and the input read rate beside the box's read-only stream rate."""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import wordpiece_model as wm
    from custrings_amd import wordpiece

    rates = (C.c_double * 6)()
    _lib.check(L.cs_box_rates(2048, 3, None, rates))
    print(json.dumps({"config": "WP box", "read_GBps": round(rates[1] * 1e3, 1)}), flush=True)
    rows = int(2_000_000 * a.scale)
    long_rows = max(int(20_000 * a.scale), 64)
    rng = np.random.default_rng(SEED)
    lens = rng.integers(3600, 4600, size=long_rows)
    offs = np.zeros(long_rows + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    text = rng.integers(97, 123, size=int(offs[-1]), dtype=np.uint8)
    text[rng.integers(0, 6, size=text.size) == 0] = 32
    # 30 000 entries: the specials, every printable ASCII byte whole and as a continuation, runs of 2..4 of a-z0-9 either way
    big = ["[UNK]", "[CLS]", "[SEP]", "[PAD]"] + [chr(c) for c in range(33, 127)] + ["##" + chr(c) for c in range(33, 127)]
    seen = set(big)
    letters = "abcdefghijklmnopqrstuvwxyz0123456789"
    while len(big) < 30000:
        run = "".join(letters[i] for i in rng.integers(0, 26 if rng.integers(0, 4) else 36, size=int(rng.integers(2, 5))))
        e = run if rng.integers(0, 2) else "##" + run
        if e not in seen:
            seen.add(e)
            big.append(e)
    vocabs = [("30000", wordpiece.vocabulary(nvstrings.to_device(big))),
              ("300", wordpiece.vocabulary(nvstrings.to_device([e.decode() for e in wm.make_vocab(300, 11)])))]
    cols = [("C3", lambda: synth(3, rows)), ("C5", lambda: synth(5, rows)), ("4KB", lambda: nvstrings.from_offsets64(text, offs, long_rows, None))]
    for name, make in cols:
        col = make()
        n, nb = col.size(), nbytes(col)
        for vname, v in vocabs:
            d_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            total = C.c_int64()
            _lib.check(L.cs_wordpiece_count(col.m_cptr, v.m_cptr, 100, 1, d_offs.data_ptr(), 1, None, C.byref(total)))
            d_ids = torch.empty(max(total.value, 1), dtype=torch.int32, device="cuda")
            enc = torch.empty((n, 128), dtype=torch.int32, device="cuda")
            mask = torch.empty((n, 128), dtype=torch.uint8, device="cuda")
            calls = [("tokenize", lambda: wordpiece.tokenize(col, v, punct=True, devptrs=(d_ids, d_offs)), total.value),
                     ("encode 128", lambda: wordpiece.encode(col, v, 128, cls="[CLS]", sep="[SEP]", pad="[PAD]", punct=True, devptrs=(enc, mask)), None)]
            for op, fn, ids in calls:
                dt = timed(fn, reps=3)
                if ids is None:
                    ids = int(mask.sum(dtype=torch.int64).item())
                line = {"config": "WP %s vocab %s" % (name, vname), "op": op, "route": L.cs_debug_last_route().decode(), "rows": n, "bytes": nb,
                        "ids": ids, "ms": round(dt * 1e3, 3), "ids_per_s": round(ids / dt, 0), "input_GBps": round((nb + 8.125 * n) / dt / 1e9, 1),
                        "frac_of_box_read_rate": round((nb + 8.125 * n) / dt / (rates[1] * 1e12), 4)}
                if op == "tokenize":
                    line["unk_share"] = round(float((d_ids[:total.value] == v.unk_id).float().mean().item()), 4) if total.value else 0.0
                print(json.dumps(line), flush=True)
            del d_offs, d_ids, enc, mask
        del col


def run_minhash(a):
    """minhash (cs_minhash) at width 5: the C3 log-line column and the C5 column at 2M rows (x --scale) and a generated column
    of 20 000 rows of ~4 KB, at nperm 64 and 256 -- ms, (n-grams x nperm) per second, the form that ran -- and at nperm 1,
    where the input read rate is set beside the box's read-only stream rate (cs_box_rates); then the band keys of the
    256-wide signatures.  The n-gram count comes from len(): max(chars - 4, 1) for a row with a character."""
    import numpy as np

    from custrings_amd import minhash

    rates = (C.c_double * 6)()
    _lib.check(L.cs_box_rates(2048, 3, None, rates))
    print(json.dumps({"config": "MINHASH box", "read_GBps": round(rates[1] * 1e3, 1)}), flush=True)
    rows = int(2_000_000 * a.scale)
    long_rows = max(int(20_000 * a.scale), 64)
    rng = np.random.default_rng(SEED)
    lens = rng.integers(3600, 4600, size=long_rows)
    offs = np.zeros(long_rows + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    text = rng.integers(97, 123, size=int(offs[-1]), dtype=np.uint8)
    text[rng.integers(0, 6, size=text.size) == 0] = 32
    cols = [("C3", lambda: synth(3, rows)), ("C5", lambda: synth(5, rows)), ("4KB", lambda: nvstrings.from_offsets64(text, offs, long_rows, None))]
    for name, make in cols:
        col = make()
        n = col.size()
        nch = torch.empty(n, dtype=torch.int32, device="cuda")
        col.len(nch.data_ptr())
        grams = int(torch.where(nch >= 5, nch - 4, nch.clamp(0, 1)).sum(dtype=torch.int64).item())
        for nperm in (1, 64, 256):
            pa, pb = minhash.permutations(nperm, 0)
            out = torch.empty((n, nperm), dtype=torch.int32, device="cuda")
            dt = timed(lambda: minhash.minhash(col, width=5, seed=0, a=pa, b=pb, devptr=out), reps=3)
            line = {"config": "MINHASH " + name, "op": "minhash width 5 nperm %d" % nperm, "route": L.cs_debug_last_route().decode(), "rows": n,
                    "bytes": nbytes(col), "ngrams": grams, "ms": round(dt * 1e3, 3), "gram_perms_per_s": round(grams * nperm / dt, 0)}
            if nperm == 1:
                line["input_GBps"] = round((nbytes(col) + 8.125 * n) / dt / 1e9, 1)
                line["frac_of_box_read_rate"] = round((nbytes(col) + 8.125 * n) / dt / (rates[1] * 1e12), 4)
            print(json.dumps(line), flush=True)
            if nperm == 256:
                keys = torch.empty((n, 32), dtype=torch.int64, device="cuda")
                dt = timed(lambda: minhash.band_keys(out, 32, devptr=keys), reps=3)
                print(json.dumps({"config": "MINHASH " + name, "op": "band_keys 256 -> 32", "rows": n, "ms": round(dt * 1e3, 3)}), flush=True)
            del out
        del col


def run_stats(a):
    """compute_statistics / get_info (cs_column_statistics) on the C2, C3 and C5 columns at 20M rows (x --scale): (a) the fused
    pass for the length and class figures, (b) what gives the same figures without it -- len, byte_count and isspace /
    isdigit / isupper / islower, summed -- (c) the pass with the histogram, in each layout of CS_STATS_HIST (1 per-workgroup
    LDS bins, 2 per-wave bins, 3 per-workgroup bins behind the wave's leader-match step), and the whole call with the distinct
    count.  Beside them the box's read-only stream rate (cs_box_rates) and each pass's share of it at one read of the column
    (chars, offsets, validity)."""
    rates = (C.c_double * 6)()
    _lib.check(L.cs_box_rates(2048, 3, None, rates))
    read_rate = rates[1] * 1e12
    print(json.dumps({"config": "STATS box", "read_GBps": round(rates[1] * 1e3, 1)}), flush=True)
    rows = int(20_000_000 * a.scale)
    for kind, name in ((2, "C2"), (3, "C3"), (5, "C5")):
        col = synth(kind, rows)
        one_read = nbytes(col) + 8.125 * rows
        res32 = torch.empty(rows, dtype=torch.int32, device="cuda")
        res8 = torch.empty(rows, dtype=torch.uint8, device="cuda")

        def line(op, fn, passes=1, reps=5):
            dt = timed(fn, reps=reps)
            print(json.dumps({"config": "STATS " + name, "op": op, "rows": rows, "ms": round(dt * 1e3, 3), "chars_reads": passes,
                              "frac_of_box_read_rate_at_one_read": round(one_read / dt / read_rate, 4)}), flush=True)
            return dt

        fused = line("(a) fused pass: lengths + classes", lambda: nvstrings.column_statistics(col, 3))
        route = L.cs_debug_last_route().decode()
        today = [("len", lambda: col.len(res32.data_ptr())), ("byte_count", lambda: col.byte_count(res32.data_ptr(), True)),
                 ("isspace", lambda: col.isspace(res8.data_ptr())), ("isdigit", lambda: col.isdigit(res8.data_ptr())),
                 ("isupper", lambda: col.isupper(res8.data_ptr())), ("islower", lambda: col.islower(res8.data_ptr()))]
        total = sum(line("(b) part: " + op, fn) for op, fn in today)
        print(json.dumps({"config": "STATS " + name, "op": "(b) len + byte_count + isspace + isdigit + isupper + islower", "rows": rows,
                          "ms": round(total * 1e3, 3), "fused_route": route, "fused_over_separate": round(fused / total, 3)}), flush=True)
        for layout in (1, 2, 3):
            L.cs_config_set(b"CS_STATS_HIST", str(layout).encode())
            line("(c) fused pass + histogram, CS_STATS_HIST=%d" % layout, lambda: nvstrings.column_statistics(col, 7))
            line("    histogram alone, CS_STATS_HIST=%d" % layout, lambda: nvstrings.column_statistics(col, 4))
        L.cs_config_set(b"CS_STATS_HIST", None)
        line("whole call: pass + histogram + distinct count (get_info)", lambda: col.get_info(), reps=2)
        del col


def run_c2(a, ov):
    # ---- C2: 10M x 64 chars, lower + strip + split(' ')
    rows = int(10_000_000 * a.scale)
    c2 = synth(2, rows)
    b = nbytes(c2)
    low = c2.lower()
    report("C2", "lower", rows, b, 2 * b + 2 * ov * rows, timed(lambda: c2.lower()))
    st = low.strip()
    report("C2", "strip", rows, nbytes(low), nbytes(low) + nbytes(st) + 2 * ov * rows, timed(lambda: low.strip()))
    cols = st.split(" ")
    out_b = sum(nbytes(c) for c in cols)
    report("C2", "split(' ')", rows, nbytes(st), nbytes(st) + ov * rows + out_b + sum(col_ov(c) for c in cols) * rows, timed(lambda: st.split(" ")))
    report("C2", "upper", rows, b, 2 * b + 2 * ov * rows, timed(lambda: c2.upper()))
    res = torch.empty(rows, dtype=torch.int32, device="cuda")
    report("C2", "find('é')", rows, b, b + ov * rows + 4 * rows, timed(lambda: c2.find("é", devptr=res.data_ptr())))
    resb = torch.empty(rows, dtype=torch.uint8, device="cuda")
    report("C2", "contains('ab', regex=False)", rows, b, b + ov * rows + rows, timed(lambda: c2.contains("ab", regex=False, devptr=resb.data_ptr())))
    rl = c2.replace("a", "xx", regex=False)
    report("C2", "replace('a','xx') literal", rows, b, b + nbytes(rl) + 2 * ov * rows, timed(lambda: c2.replace("a", "xx", regex=False)))
    rs = c2.replace("ab", "x", regex=False)
    report("C2", "replace('ab','x') literal", rows, b, b + nbytes(rs) + 2 * ov * rows, timed(lambda: c2.replace("ab", "x", regex=False)))
    # ingest / egress through the reference's Arrow boundary (int32 offsets + bitmask, device buffers):
    # create_offsets (NVStrings.cu:402-482), create_from_offsets (NVStringsImpl.cu:399-444), byte_count
    chars = torch.empty(b + 64, dtype=torch.uint8, device="cuda")
    offs = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
    mask = torch.empty((rows + 7) // 8 + 8, dtype=torch.uint8, device="cuda")
    report("C2", "egress to_offsets (device, int32)", rows, b, 2 * b + (ov + 4.125) * rows,
           timed(lambda: c2.to_offsets(chars.data_ptr(), offs.data_ptr(), mask.data_ptr(), bdevmem=True)))
    report("C2", "ingest from_offsets (device, int32)", rows, b, 2 * b + (ov + 4.125) * rows,
           timed(lambda: nvstrings.from_offsets(chars.data_ptr(), offs.data_ptr(), rows, mask.data_ptr(), 0, bdevmem=True)))
    lens = torch.empty(rows, dtype=torch.int32, device="cuda")
    report("C2", "byte_count (device)", rows, b, (ov + 4) * rows, timed(lambda: c2.byte_count(lens.data_ptr(), bdevmem=True)))
    del c2, low, st, cols, rl, rs, chars, offs, mask, lens



def run_c3(a, ov):
    # ---- C3: 100M log lines, contains_re + replace_re + split
    rows = int(100_000_000 * a.scale)
    c3 = synth(3, rows)
    b = nbytes(c3)
    resb = torch.empty(rows, dtype=torch.uint8, device="cuda")
    report("C3", "contains_re(IPv4)", rows, b, b + ov * rows + rows, timed(lambda: c3.contains(IPV4, devptr=resb.data_ptr())))
    resi = torch.empty(rows, dtype=torch.int32, device="cuda")
    report("C3", "count_re(IPv4)", rows, b, b + ov * rows + 4 * rows, timed(lambda: c3.count(IPV4, devptr=resi.data_ptr())))
    fa = c3.findall(IPV4)
    report("C3", "findall(IPv4) -> %d columns" % len(fa), rows, b, b + ov * rows + sum(nbytes(c) for c in fa) + sum(col_ov(c) for c in fa) * rows,
           timed(lambda: c3.findall(IPV4)))
    del fa
    report("C3", "extract((\\d+)\\.(\\d+)\\.\\d+\\.(\\d+) ), 3 groups", rows, b, b + ov * rows + 3 * (ov * rows) + 6 * rows,
           timed(lambda: c3.extract(r"(\d+)\.(\d+)\.\d+\.(\d+) "), reps=2))
    bk = c3.replace_with_backrefs(r"(\d+)\.(\d+)\.(\d+)\.(\d+)", r"\4.\3.\2.\1")
    report("C3", "replace_with_backrefs(IPv4 octets reversed)", rows, b, b + nbytes(bk) + 2 * ov * rows,
           timed(lambda: c3.replace_with_backrefs(r"(\d+)\.(\d+)\.(\d+)\.(\d+)", r"\4.\3.\2.\1"), reps=2))
    del bk
    rep = c3.replace(IPV4, "<IP>")
    report("C3", "replace_re(IPv4,'<IP>')", rows, b, b + nbytes(rep) + 2 * ov * rows, timed(lambda: c3.replace(IPV4, "<IP>")))
    del rep
    # BASELINE.md section 3's secondary pattern (26 instructions) and the reference gtest's alternation of word-bounded
    # literals (cpp/tests/test_replace.cpp:41), each with the executor it takes (cs_regex_engine)
    for name, pat, repl in (("IPv4 with \\b and {1,3}", IPV4B, "<IP>"), ("(\\bin\\b)|(\\ba\\b)|(\\bthe\\b)", GTEST, "=")):
        re = nvstrings._compile(pat)
        e = int(L.cs_regex_engine(re))
        how = ("tagged DFA, %d states, %d threads%s" % (e >> 16, (e >> 8) & 15, ", unit scan offered" if e & 2 else "")) if e & 1 else "list simulator"
        ninst = int(L.cs_regex_inst_count(re))
        L.cs_regex_destroy(re)
        report("C3", "contains_re(%s) [%d instructions; %s]" % (name, ninst, how), rows, b, b + ov * rows + rows,
               timed(lambda: c3.contains(pat, devptr=resb.data_ptr())))
        report("C3", "match(%s)" % name, rows, b, b + ov * rows + rows, timed(lambda: c3.match(pat, devptr=resb.data_ptr())))
        cnt32 = torch.zeros(rows, dtype=torch.int32, device="cuda")
        report("C3", "count_re(%s)" % name, rows, b, b + ov * rows + 4 * rows, timed(lambda: c3.count(pat, devptr=cnt32.data_ptr())))
        del cnt32
        rep = c3.replace(pat, repl)
        route = L.cs_debug_last_route().decode()
        report("C3", "replace_re(%s,'%s') [route: %s]" % (name, repl, route), rows, b, b + nbytes(rep) + 2 * ov * rows, timed(lambda: c3.replace(pat, repl), reps=2))
        del rep
    # a small set in a `+` loop: candidates in a good share of the bytes (the bit-parallel form, regex_bits.h)
    rep = c3.replace(r"[aeiou]+", "*")
    report("C3", "replace_re([aeiou]+,'*') [route: %s]" % L.cs_debug_last_route().decode(), rows, b, b + nbytes(rep) + 2 * ov * rows, timed(lambda: c3.replace(r"[aeiou]+", "*"), reps=2))
    del rep
    report("C3", "match(IPv4)", rows, b, b + ov * rows + rows, timed(lambda: c3.match(IPV4, devptr=resb.data_ptr())))
    rc = c3.rsplit(" ")
    report("C3", "rsplit(' ') (no limit: the split kernels)", rows, b, b + ov * rows + sum(nbytes(c) for c in rc) + sum(col_ov(c) for c in rc) * rows,
           timed(lambda: c3.rsplit(" ")))
    del rc
    rc = c3.rsplit(" ", 3)
    report("C3", "rsplit(' ', 3) (the split kernels, the row's first delimiters struck from the mask)", rows, b, b + ov * rows + sum(nbytes(c) for c in rc) + sum(col_ov(c) for c in rc) * rows,
           timed(lambda: c3.rsplit(" ", 3), reps=2))
    del rc
    cols = c3.split(" ")
    out_b = sum(nbytes(c) for c in cols)
    out_ov = sum(col_ov(c) for c in cols)
    del cols
    report("C3", "split(' ')", rows, b, b + ov * rows + out_b + out_ov * rows, timed(lambda: c3.split(" ")))
    cols = c3.split()
    out_b = sum(nbytes(c) for c in cols)
    out_ov = sum(col_ov(c) for c in cols)
    del cols
    report("C3", "split() whitespace", rows, b, b + ov * rows + out_b + out_ov * rows, timed(lambda: c3.split(), reps=2))
    # first touch: a fresh column's first op also pays the column's metadata passes (largest 64-row span, longest row, byte
    # classes: kept on the immutable column afterwards) -- the steady-state figures above do not show them
    def fresh_first(op):
        c = synth(3, rows)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = op(c)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del r, c
        return dt
    fresh_first(lambda c: c.split(" "))  # (kernel load, allocator)
    report("C3", "split(' '), FIRST op on a fresh column", rows, b, b + ov * rows + out_b + out_ov * rows, fresh_first(lambda c: c.split(" ")))
    rep = c3.replace(IPV4, "<IP>")
    # (once unmeasured: with no block of the output's size in the pool the call pays a hipMalloc of gigabytes -- 120 ms -- which is
    # the allocator's first touch, not the column's; tools/probe_fresh_first.py)
    fresh_first(lambda c: c.replace(IPV4, "<IP>"))
    report("C3", "replace_re(IPv4,'<IP>'), FIRST op on a fresh column", rows, b, b + nbytes(rep) + 2 * ov * rows, fresh_first(lambda c: c.replace(IPV4, "<IP>")))
    del rep
    del c3, resb, resi



def run_c4(a, ov):
    # ---- C4: 16-char tokens, category build (per-GPU shard of the 1B-row config: 125M rows)
    rows = int(125_000_000 * a.scale)
    # (K = 2^40 names of the log-uniform generator: nearly every row is its own key -- BASELINE.md section 3's "K = 100M" case)
    for K in (1000, 1 << 20, 1 << 27, 1 << 40):
        c4 = synth(4, rows, K)
        b = nbytes(c4)
        cat = nvcategory.from_strings(c4)
        nk = cat.keys_size()
        del cat
        report("C4", "category build K=%d (%d distinct keys)" % (K, nk), rows, b, b + ov * rows + 4 * rows, timed(lambda: nvcategory.from_strings(c4), reps=2))
        del c4



def run_c5(a, ov):
    # ---- C5: tweet-like rows, tokenize + bigrams (per-GPU shard: 62.5M rows)
    rows = int(62_500_000 * a.scale)
    c5 = synth(5, rows)
    b = nbytes(c5)
    tok = nvtext.tokenize(c5)
    t = tok.size()
    report("C5", "tokenize", rows, b, b + ov * rows + nbytes(tok) + ov * t, timed(lambda: nvtext.tokenize(c5), reps=2))
    # a single class in a `+` loop on rows of 40-150 bytes (beyond the 96-bit masks): byte-parallel compaction (cs_runs.hip)
    rp = c5.replace(r"[aeiou]+", "*")
    report("C5", "replace_re([aeiou]+,'*') [route: %s]" % L.cs_debug_last_route().decode(), rows, b, b + nbytes(rp) + 2 * ov * rows, timed(lambda: c5.replace(r"[aeiou]+", "*"), reps=2))
    del rp
    del c5
    rep = c5.replace(r"[aeiou]+", "*") if False else None
    ng = nvtext.ngrams(tok, 2, "_")
    report("C5", "ngrams(2)", t, nbytes(tok), nbytes(tok) + ov * t + nbytes(ng) + ov * ng.size(), timed(lambda: nvtext.ngrams(tok, 2, "_"), reps=2))


def run_conv(a, ov):
    # ---- the conversion ops (convert.cu) at 100M rows, on the route the library picks and with CS_CONVERT_ROWWISE=1.
    # Parse: (L + 8.125) read + the result written per row; format: the value (+ 1/8 mask bit) read + (L' + 8.125) written.
    rows = int(100_000_000 * a.scale)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    i32 = torch.randint(-(1 << 31), (1 << 31) - 1, (rows,), dtype=torch.int32, device="cuda", generator=gen)
    i64 = torch.randint(-(1 << 63), (1 << 63) - 1, (rows,), dtype=torch.int64, device="cuda", generator=gen)
    f32 = (torch.randn(rows, device="cuda", generator=gen) * 1e3).float()
    f64 = torch.randn(rows, device="cuda", generator=gen, dtype=torch.float64) * 1e6
    bools = torch.randint(0, 2, (rows,), dtype=torch.uint8, device="cuda", generator=gen)
    c3, c4 = synth(3, rows), synth(4, rows, 1000)
    ip = c3.split(" ")[2]
    itos_col, dtos_col = nvstrings.itos(i32, bdevmem=True), nvstrings.dtos(f64, bdevmem=True)
    out = {w: torch.empty(rows, dtype=t, device="cuda") for w, t in ((1, torch.uint8), (4, torch.int32), (8, torch.int64))}
    parse = (("C3", "hash", c3, 4), ("C4", "hash", c4, 4), ("C3 field 3", "ip2int", ip, 4), ("itos output", "stoi", itos_col, 4),
             ("dtos output", "stod", dtos_col, 8))
    fmt = (("itos", i32, 4), ("ltos", i64, 8), ("ftos", f32, 4), ("dtos", f64, 8), ("int2ip", i32, 4), ("from_booleans", bools, 1))
    for route in ("default", "rowwise"):
        if route == "rowwise":
            L.cs_config_set(b"CS_CONVERT_ROWWISE", b"1")
        for cfg, op, col, w in parse:
            b = nbytes(col)
            fn = getattr(col, op)
            dt = timed(lambda: fn(devptr=out[w].data_ptr()))
            report("CONV %s [%s]" % (cfg, L.cs_debug_last_route().decode()), op, rows, b, b + ov * rows + w * rows, dt)
        for op, vals, w in fmt:
            res = getattr(nvstrings, op)(vals, bdevmem=True)
            b = nbytes(res)
            dt = timed(lambda: getattr(nvstrings, op)(vals, bdevmem=True), reps=2)
            report("CONV seeded values [%s]" % L.cs_debug_last_route().decode(), op, rows, w * rows, w * rows + b + col_ov(res) * rows, dt)
            del res
    L.cs_config_set(b"CS_CONVERT_ROWWISE", None)


def run_ts(a):
    # ---- the timestamp conversions (datetime.cu) at 100M rows in the default format ("%Y-%m-%dT%H:%M:%SZ", 20 bytes a row).
    # Parse: the chars + the offsets read, the int64 written; format: the int64 (+ 1/8 mask bit) read, the chars + the
    # offsets (+ validity) written.  Both routes / both writers: the default and CS_CONVERT_ROWWISE=1.
    rows = int(100_000_000 * a.scale)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    secs = torch.randint(0, 253402300799, (rows,), dtype=torch.int64, device="cuda", generator=gen)
    ms = secs * 1000 + torch.randint(0, 1000, (rows,), dtype=torch.int64, device="cuda", generator=gen)
    nulls = torch.randint(0, 256, ((rows + 7) // 8,), dtype=torch.uint8, device="cuda", generator=gen)
    col = nvstrings.int2timestamp(secs, bdevmem=True)
    out = torch.empty(rows, dtype=torch.int64, device="cuda")
    for route in ("default", "rowwise"):
        L.cs_config_set(b"CS_CONVERT_ROWWISE", b"1" if route == "rowwise" else None)
        b = nbytes(col)
        dt = timed(lambda: col.timestamp2int(devptr=out.data_ptr()))
        report("TS default format [%s]" % L.cs_debug_last_route().decode(), "timestamp2int(s)", rows, b, b + col_ov(col) * rows + 8 * rows, dt)
        for units, vals in (("s", secs), ("ms", ms)):
            for nl in (None, nulls):
                res = nvstrings.int2timestamp(vals, nulls=nl, units=units, bdevmem=True)
                b = nbytes(res)
                dt = timed(lambda: nvstrings.int2timestamp(vals, nulls=nl, units=units, bdevmem=True), reps=3)
                cfg = "TS seeded values%s [%s]" % (" + nulls" if nl is not None else "", L.cs_debug_last_route().decode())
                report(cfg, "int2timestamp(%s)" % units, rows, 8 * rows, 8 * rows + (0.125 * rows if nl is not None else 0) + b + col_ov(res) * rows, dt)
                del res
    L.cs_config_set(b"CS_CONVERT_ROWWISE", None)


def run_pad(a):
    # ---- the substring / padding / wrapping ops (substr.cu, pad.cu, modify.cu) on 100M rows of C3 and C2, on both routes (the
    # default and CS_PAD_ROWWISE=1).  Algorithmic bytes: the chars + the offsets + the validity read, the chars + the offsets
    # written (wrap shares the extents: its chars only).
    rows = int(100_000_000 * a.scale)
    ops = [("slice(2,12)", lambda c: c.slice(2, 12)), ("get(0)", lambda c: c.get(0)), ("ljust(100)", lambda c: c.ljust(100)),
           ("zfill(20)", lambda c: c.zfill(20)), ("repeat(2)", lambda c: c.repeat(2)), ("wrap(20)", lambda c: c.wrap(20)),
           ("slice_replace(2,5,'<>')", lambda c: c.slice_replace(2, 5, "<>"))]
    for kind, name in ((3, "C3"), (2, "C2")):
        col = synth(kind, rows)
        b = nbytes(col)
        for route in ("default", "rowwise"):
            L.cs_config_set(b"CS_PAD_ROWWISE", b"1" if route == "rowwise" else None)
            for op, fn in ops:
                res = fn(col)
                got_route = L.cs_debug_last_route().decode()
                w = nbytes(res) + (0 if op.startswith("wrap") else 8 * rows)
                dt = timed(lambda: fn(col), reps=3)
                report("PAD %s 100M [%s]" % (name, got_route), op, rows, b, b + 8.125 * rows + w, dt)
                del res
        del col
    L.cs_config_set(b"CS_PAD_ROWWISE", None)


def run_chr(a):
    # ---- the character-type predicates (attrs.cu) and swapcase / capitalize / title (case.cu) on 100M rows, on both routes
    # (the default, then CS_CONVERT_ROWWISE=1 for the predicates and CS_CASE_ROWWISE=1 for the case ops).  Algorithmic bytes:
    # predicates L + 8.125 read and 1 written a row (is_empty: 8.125 read, 1 written); case ops L + 8.125 read and L written
    # (the extents are shared).  `hash` (same staging, every byte walked) and `lower` (same bytes moved) run beside them.
    rows = int(100_000_000 * a.scale)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    i32 = torch.randint(0, (1 << 31) - 1, (rows,), dtype=torch.int32, device="cuda", generator=gen)
    out8 = torch.empty(rows, dtype=torch.uint8, device="cuda")
    out32 = torch.empty(rows, dtype=torch.int32, device="cuda")
    preds = ["isalnum", "isalpha", "isdigit", "isspace", "isdecimal", "isnumeric", "islower", "isupper", "is_empty"]
    cols = (("C3", synth(3, rows), preds), ("C4", synth(4, rows, 1000), ["isalpha", "isalnum", "islower"]),
            ("itos output", nvstrings.itos(i32, bdevmem=True), ["isdigit", "isdecimal"]))
    del i32
    for route in ("default", "rowwise"):
        L.cs_config_set(b"CS_CONVERT_ROWWISE", b"1" if route == "rowwise" else None)
        for cfg, col, ops in cols:
            b = nbytes(col)
            for op in ops + ["hash"]:
                fn = getattr(col, op)
                o, w = (out32, 4) if op == "hash" else (out8, 1)
                dt = timed(lambda: fn(devptr=o.data_ptr()))
                n = o.count_nonzero().item() if op != "hash" else -1
                alg = (0 if op == "is_empty" else b) + 8.125 * rows + w * rows
                report("CHR %s 100M [%s] true=%d" % (cfg, L.cs_debug_last_route().decode(), n), op, rows, b, alg, dt)
    L.cs_config_set(b"CS_CONVERT_ROWWISE", None)
    del cols
    for kind, name in ((3, "C3"), (2, "C2")):
        col = synth(kind, rows)
        b = nbytes(col)
        for route in ("default", "rowwise"):
            L.cs_config_set(b"CS_CASE_ROWWISE", b"1" if route == "rowwise" else None)
            for op in ("lower", "swapcase", "capitalize", "title"):
                fn = getattr(col, op)
                dt = timed(fn, reps=3)
                got_route = L.cs_debug_last_route().decode() if op != "lower" else ("rows" if route == "rowwise" else "tile")
                wr = (8 * rows) if route == "rowwise" else 0  # (the two-pass kernels write offsets of their own)
                report("CHR %s 100M [%s]" % (name, got_route), op, rows, b, 2 * b + 8.125 * rows + wr, dt)
        del col
    L.cs_config_set(b"CS_CASE_ROWWISE", None)


def run_url(a):
    # ---- url_encode / url_decode / translate / fillna (urlencode.cu, modify.cu:302-489) on the C3 and C5 columns, on both routes
    # (the default, then CS_RECODE_ROWWISE=1; fillna has one).  Bytes: the chars + offsets + validity read, the chars + offsets
    # written.  Beside them, from the same run: the box's copy rate (cs_box_rates) and slice / lower on the same column.
    # url_decode runs on url_encode's output; translate with an ASCII table (e -> E, ' ' -> '_', '.' dropped) and with one that
    # changes widths (' ' -> U+20AC, 'e' -> U+00E9).
    rates = (C.c_double * 6)()
    _lib.check(L.cs_box_rates(2048, 3, None, rates))
    print(json.dumps({"config": "URL box", "copy_GBps": round(rates[0] * 1e3, 1), "read_GBps": round(rates[1] * 1e3, 1),
                      "write_GBps": round(rates[2] * 1e3, 1)}), flush=True)
    ascii_t = {ord("e"): ord("E"), ord(" "): ord("_"), ord("."): None}
    wide_t = {ord(" "): 0x20AC, ord("e"): 0xE9}
    for kind, name, rows in ((3, "C3", int(100_000_000 * a.scale)), (5, "C5", int(62_500_000 * a.scale))):
        col = synth(kind, rows)
        b = nbytes(col)

        def line(cfg, op, src, fn, extra=0):
            res = fn()
            w = nbytes(res) + 8 * rows
            route = L.cs_debug_last_route().decode()
            del res
            dt = timed(fn, reps=3)
            report("URL %s %s [%s]" % (name, cfg, route), op, rows, nbytes(src), nbytes(src) + 8.125 * rows + extra + w, dt)

        enc = col.url_encode()
        for route in ("default", "rowwise"):
            L.cs_config_set(b"CS_RECODE_ROWWISE", b"1" if route == "rowwise" else None)
            line(route, "url_encode", col, lambda: col.url_encode())
            line(route, "url_decode (of url_encode)", enc, lambda: enc.url_decode())
            line(route, "translate (3 ASCII keys)", col, lambda: col.translate(ascii_t))
            line(route, "translate (2 keys, 1 -> 3 / 2 bytes)", col, lambda: col.translate(wide_t))
        L.cs_config_set(b"CS_RECODE_ROWWISE", None)
        line("default", "fillna('-')", col, lambda: col.fillna("-"))
        line("default", "fillna(column)", col, lambda: col.fillna(enc), extra=0.125 * rows)
        dt = timed(lambda: col.slice(2, 12), reps=3)
        report("URL %s neighbour [%s]" % (name, L.cs_debug_last_route().decode()), "slice(2,12)", rows, b, b + 8.125 * rows + nbytes(col.slice(2, 12)) + 8 * rows, dt)
        dt = timed(lambda: col.lower(), reps=3)
        report("URL %s neighbour" % name, "lower", rows, b, 2 * b + 8.125 * rows, dt)
        del col, enc


def run_txt(a):
    # ---- contains_strings / strings_counts / edit_distance / porter_stemmer_measure / scatter_count (NVText.cu, edit_distance.cu,
    # stemmer.cu) on the C3 and C2 columns at 10M rows, on both routes (the default, then CS_TEXT_ROWWISE=1); `hash` beside them as
    # the bandwidth-bound neighbour.  Algorithmic bytes: L + 8.125 read a row and the results written (M values a row for the
    # matches; scatter_count: the gather's bytes).  The scalar edit_distance at targets of 8, 64 and 65 characters: 65 takes the
    # dynamic program on either route.
    rows = int(10_000_000 * a.scale)
    words = ["the", "er", "a", "GET", "in", "10", "e ", "on", ".1", "st", "al", "to", "ng", "0 ", "ha", "it"]
    t2, t32 = nvstrings.to_device(words[:2]), nvstrings.to_device(words + [w + "x" for w in words])
    text = "GET /index.html HTTP/1.1 200 the quick brown fox jumps over the lazy dog again"
    out8 = torch.empty(rows * 32, dtype=torch.uint8, device="cuda")
    out32 = torch.empty(rows * 32, dtype=torch.int32, device="cuda")
    cnt = (torch.arange(rows, dtype=torch.int32, device="cuda") % 3).contiguous()
    for kind, name in ((3, "C3"), (2, "C2")):
        col = synth(kind, rows)
        b = nbytes(col)
        for route in ("default", "rowwise"):
            L.cs_config_set(b"CS_TEXT_ROWWISE", b"1" if route == "rowwise" else None)

            def line(op, call, written, reps=3):
                dt = timed(call, reps=reps)
                report("TXT %s 10M [%s]" % (name, L.cs_debug_last_route().decode()), op, rows, b, b + 8.125 * rows + written, dt)

            if route == "default":
                dt = timed(lambda: col.hash(devptr=out32.data_ptr()))
                report("TXT %s 10M [%s]" % (name, L.cs_debug_last_route().decode()), "hash", rows, b, b + 12.125 * rows, dt)
            for tg, M in ((t2, 2), (t32, 32)):
                line("contains_strings M=%d" % M, lambda: _lib.check(L.cs_contains_strings(col.m_cptr, tg.m_cptr, out8.data_ptr(), 1, None)), M * rows)
                line("strings_counts M=%d" % M, lambda: _lib.check(L.cs_strings_counts(col.m_cptr, tg.m_cptr, out32.data_ptr(), 1, None)), 4 * M * rows)
            for chars in (8, 64, 65):
                target = text[:chars].encode()
                line("edit_distance target=%d" % chars, lambda: _lib.check(L.cs_edit_distance(col.m_cptr, target, 0, out32.data_ptr(), 1, None)),
                     4 * rows, reps=1)
            line("edit_distance_column (self)", lambda: _lib.check(L.cs_edit_distance_column(col.m_cptr, col.m_cptr, 0, out32.data_ptr(), 1, None)),
                 b + 8.125 * rows + 4 * rows, reps=1)
            line("porter_stemmer_measure", lambda: _lib.check(L.cs_porter_stemmer_measure(col.m_cptr, None, None, out32.data_ptr(), 1, None)), 4 * rows)
            if route == "default":
                def scatter():
                    o = C.c_void_p()
                    _lib.check(L.cs_scatter_count(col.m_cptr, cnt.data_ptr(), 1, None, C.byref(o)))
                    return nvstrings.nvstrings(o.value)

                line("scatter_count (0/1/2)", scatter, 4 * rows + b + 2 * 8.125 * rows)
        del col
    L.cs_config_set(b"CS_TEXT_ROWWISE", None)




def run_csv(a):
    """from_csv_buffer on generated text of 2M lines (x --scale): C3-like log lines (one column, no quotes) and a 9-column shape
    like the reference's tweets file (column 7 quoted, "" pairs inside).  Per shape: the line-start kernels and the field locator
    by themselves (cs_prof: HIP events around their launches; the locator's figure includes its tile plan), the whole call on
    device bytes and on host bytes (with its upload), and to_device of the same rows as a Python list.  Beside them, from the
    same run, the box's read-only stream rate (cs_box_rates)."""
    import numpy as np

    rates = (C.c_double * 6)()
    _lib.check(L.cs_box_rates(2048, 3, None, rates))
    print(json.dumps({"config": "CSV box", "copy_GBps": round(rates[0] * 1e3, 1), "read_GBps": round(rates[1] * 1e3, 1),
                      "write_GBps": round(rates[2] * 1e3, 1)}), flush=True)
    lines = int(2_000_000 * a.scale)
    words = ["alpha", "GET", "/index.html", "HTTP/1.1", "200", "10.0.0.7", "Mozilla/5.0", "nice to know", "paper is the best", "http://t.co/x"]
    log = ["%d.%d.%d.%d - - [10/Oct/2000:13:55:%02d -0700] \"GET /%s/%s HTTP/1.1\" %d %d" % (k % 223 + 1, k % 251, k % 241, k % 239, k % 60, words[k % 10], words[k % 7], 200 + k % 5, k * 37 % 9973)
           for k in range(1000)]
    tweets = ["%d,%d,%s,%s,%d,%d,%s,\"@%s %s, and a \"\"%s\"\" page of %d words\",%s" % (k, k * 7919 % 100003, words[k % 10], words[k % 3], k % 97, k % 89, words[k % 5], words[k % 4], words[7 + k % 2], words[k % 6],
                                                                                 k % 53, words[k % 8]) for k in range(1000)]
    for name, block, column in (("log lines", log, 0), ("9 columns, quoted", tweets, 7)):
        text = ("h0,h1,h2,h3,h4,h5,h6,h7,h8\n" + "\n".join(block * max(1, lines // 1000)) + "\n").encode()
        n = len(text)
        host = np.frombuffer(text, dtype=np.uint8)
        dev = torch.from_numpy(host.copy()).cuda()
        col = nvstrings.from_csv_buffer(dev, column)
        rows, out_b = col.size(), nbytes(col)
        L.cs_prof_reset()
        L.cs_prof_enable(1)
        reps = 3
        for _ in range(reps):
            nvstrings.from_csv_buffer(dev, column)
        torch.cuda.synchronize()
        L.cs_prof_enable(0)
        for kern, what in ((b"k_csv_line_starts", "line starts (summary + scan + write)"), (b"k_csv_fields", "field locator (with its tile plan)")):
            ms, k = C.c_double(), C.c_int64()
            L.cs_prof_get(kern, C.byref(ms), C.byref(k))
            dt = ms.value / reps / 1e3
            print(json.dumps({"config": "CSV " + name, "op": what, "rows": rows, "text_bytes": n, "ms": round(dt * 1e3, 3), "text_GBps": round(n / dt / 1e9, 1),
                              "frac_of_box_read": round(n / dt / 1e9 / (rates[1] * 1e3), 3), "route": L.cs_debug_last_route().decode()}), flush=True)
        report("CSV " + name, "from_csv_buffer (device bytes)", rows, n, n + out_b + 8.125 * rows, timed(lambda: nvstrings.from_csv_buffer(dev, column)))
        report("CSV " + name, "from_csv_buffer (host bytes, with the upload)", rows, n, n + out_b + 8.125 * rows, timed(lambda: nvstrings.from_csv_buffer(host, column)))
        strs = col.to_host()
        report("CSV " + name, "to_device (the same rows as a list)", rows, out_b, out_b + 8.125 * rows, timed(lambda: nvstrings.to_device(strs), reps=1))
        del col, dev, strs


def run_num(a):
    """from_numbers on 100M rows of int32 / int64 / float64 at K = 1 000, K = 1 M and K = N distinct keys, to_numbers and
    merge_and_remap of two such categories -- and, in the same run, two yardsticks that are not the code under test:
    radix_sort_pairs64 over all N (image, row) pairs (the reference's sort-every-row on this project's sort) and the string
    cs_category_build at the same N and K.  Algorithmic bytes of the build: the rows read once, an int32 value written."""
    from custrings_amd import nvcategory

    rows = int(100_000_000 * a.scale)
    for K in (1000, 1_000_000, rows):
        K = min(K, rows)
        base = torch.randperm(rows, device="cuda") if K == rows else torch.randint(0, K, (rows,), device="cuda")
        base = base - K // 2  # negatives mixed in
        for name, code, col in (("int32", 1, base.to(torch.int32)), ("int64", 2, base.to(torch.int64)), ("float64", 4, base.to(torch.float64) * 0.5)):
            width = col.element_size()
            dt = timed(lambda: nvcategory.from_numbers(col))
            report("NUM", "from_numbers %s K=%d" % (name, K), rows, rows * width, rows * (width + 4), dt)
            dt = timed(lambda: _lib.check(L.cs_debug_numcat_sort_rows(col.data_ptr(), rows, code, 1, None)))
            report("NUM", "yardstick radix_sort_pairs64 of all rows %s K=%d" % (name, K), rows, rows * width, rows * (width + 4), dt)
            cat = nvcategory.from_numbers(col)
            out = torch.empty_like(col)
            dt = timed(lambda: cat.to_numbers(out))
            report("NUM", "to_numbers %s K=%d" % (name, K), rows, rows * 4, rows * (width + 4), dt)
            other = nvcategory.from_numbers(col + (K // 2))  # half of the keys shared
            dt = timed(lambda: cat.merge_and_remap(other))
            report("NUM", "merge_and_remap %s K=%d" % (name, K), 2 * rows, 2 * rows * 4, 2 * rows * 8, dt)
            del cat, other, out, col
        del base
        strs = synth(4, rows, K)
        dt = timed(lambda: nvcategory.from_strings(strs))
        report("NUM", "yardstick string cs_category_build K=%d" % K, rows, nbytes(strs), nbytes(strs) + rows * 4, dt)
        del strs


if __name__ == "__main__":
    main()
