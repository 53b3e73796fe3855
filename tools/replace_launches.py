"""The launches of the replace route, of the scan route, of the split route or of the span routes, case by case (dev
tool): which kernels a call starts, on what grid and with how much dynamic LDS, for every case of
tests/test_gpu_replace_forms.py (`run replace`: plus bench.py's pattern on a 1M-row generated column), of
tests/test_gpu_scan_forms.py (`run scan`: plus contains_re and count_re of that pattern on the same column), of
tests/test_gpu_split_forms.py (`run split`: plus split(' ') on that column; the single pass's cases where the library
has the experiments) or of tests/test_gpu_span_forms.py (`run spans`: plus findall, extract and replace_with_backrefs
with tools/bench_ops.py's patterns on that column) or of the category build (`run category`: the key sets of
tests/test_gpu_category_order.py on its three routes, test_gpu_category_table_growth's column from three first table
sizes, the plain slots, the radix sort at a small count, the 4.3M-row column that takes the sampled sizing, and the
generated C4 column of 1M rows at K = 1000 and 2^20).  Two builds whose listings agree start the same kernels.

    rocprofv3 --kernel-trace --output-format json -d DIR -- python tools/replace_launches.py run scan 2> DIR/stream_info.txt
    python tools/replace_launches.py list DIR > listing.txt

`run` makes the calls in a fixed order with CS_STREAM_INFO set (the library's own account of every single-pass launch, on
stderr, behind a `case` line); `list` prints the trace's dispatches in order: kernel, grid, workgroup, LDS.  The LDS is
the dispatch packet's group segment size (`dispatch_info.group_segment_size` of the JSON trace: the kernel's static LDS
plus the dynamic LDS of the launch); the CSV trace's `LDS_Block_Size` column shows 0 for a kernel whose LDS is all
dynamic, so a CSV trace is listed only when there is no JSON one, and says so.  The runtime's own copy and fill kernels
(`__amd_rocclr_*`: a hipMemcpy or hipMemset each) are folded, a run of them into one line with their numbers (the listings under profiles/replaceplan were made before
that: they show every such dispatch on a line of its own, and are otherwise what `run replace` + `list` give).
CS_LIB_PATH picks the build."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def run(table):
    import gpuutil
    import test_gpu_replace_forms as forms

    L = gpuutil.lib()
    L.check(L.lib.cs_config_set(b"CS_STREAM_INFO", b"1"))

    def call(name, switches, fn):
        sys.stderr.write("case %s\n" % name)
        sys.stderr.flush()
        for v in switches:
            L.check(L.lib.cs_config_set(v.encode(), b"1"))
        try:
            fn()
        finally:
            for v in switches:
                L.check(L.lib.cs_config_set(v.encode(), None))
        sys.stderr.write("route %s\n" % L.lib.cs_debug_last_route().decode())

    def replace(g, op, pat, repl, maxrepl):
        if op == forms.RE:
            g.replace(pat, repl, maxrepl)
        elif op == forms.LIT:
            g.replace(pat, repl, maxrepl, regex=False)
        else:
            g.replace_with_backrefs(pat, repl)

    def scan(scans, g, op, pat):  # (host results: with device results the kernels are the same, only the copy back goes)
        re = gpuutil.compile_re(pat)
        try:
            scans.call(L, op, g, re, False)
        finally:
            L.lib.cs_regex_destroy(re)

    if table == "replace":
        for name, op, pat, repl, maxrepl, kind, n, switches in forms.CASES:
            call(name, switches, lambda: replace(forms._col(kind, n)[1], op, pat, repl, maxrepl))
        bench = gpuutil.synth(3, 0, 1_000_000)
        for i in range(2):  # (the second call finds the column's metadata cached)
            call("bench-1M-%d" % i, (), lambda: replace(bench, forms.RE, forms.IPV4, "<IP>", -1))
    elif table == "split":
        import test_gpu_split_forms as splits

        def split(g, op, delim, maxsplit, switches):  # (the table's switches may carry a value: NAME=VALUE)
            pairs = [(v.split("=") + ["1"])[:2] for v in switches]
            for k, v in pairs:
                L.check(L.lib.cs_config_set(k.encode(), v.encode()))
            try:
                getattr(g, op)(delim, maxsplit)
            finally:
                for k, _ in pairs:
                    L.check(L.lib.cs_config_set(k.encode(), None))

        for name, op, delim, maxsplit, kind, n, switches in splits.CASES + (splits.SINGLE if L.lib.cs_has_experiments() else []):
            call(name, (), lambda: split(splits._col(kind, n)[1], op, delim, maxsplit, switches))
        bench = gpuutil.synth(3, 0, 1_000_000)
        for i in range(2):  # (the second call finds the column's metadata cached)
            call("bench-1M-%d" % i, (), lambda: bench.split(" "))
    elif table == "spans":
        import test_gpu_scan_forms as scans
        import test_gpu_span_forms as spans

        for name, op, pat, tmpl, kind, n, switches in spans.CASES:
            call(name, switches, lambda: spans.run(scans._col(kind, n)[1], op, pat, tmpl))
        bench = gpuutil.synth(3, 0, 1_000_000)
        # (tools/bench_ops.py's patterns)
        for op, pat, tmpl in ((spans.FINDALL, forms.IPV4, None), (spans.EXTRACT, r"(\d+)\.(\d+)\.\d+\.(\d+) ", None), (spans.BREFS, r"(\d+)\.(\d+)\.(\d+)\.(\d+)", r"\4.\3.\2.\1")):
            for i in range(2):
                call("bench-1M-%s-%d" % (op, i), (), lambda: spans.run(bench, op, pat, tmpl))
    elif table == "category":
        import random

        import test_gpu_category_order as order
        from custrings_amd import nvcategory

        def build(g, switches):  # (NAME=VALUE, or NAME for 1)
            pairs = [(v.split("=") + ["1"])[:2] for v in switches]
            for k, v in pairs:
                L.check(L.lib.cs_config_set(k.encode(), v.encode()))
            try:
                nvcategory.from_strings(g)
            finally:
                for k, _ in pairs:
                    L.check(L.lib.cs_config_set(k.encode(), None))

        # the order test's key sets (9000 rows, 5 % of them null) on its three routes
        for kind in order.KEY_SETS:
            for count in (2048, 2049, 6000):
                rnd = random.Random("%s %d" % (kind, count))
                g = order.column(order.make_rows(order.KEY_SETS[kind](count, rnd), True, rnd))
                for route, switch in order.ROUTES:
                    call("%s-%d-%s" % (kind, count, route), (), lambda: build(g, [switch] if switch else []))
        # test_gpu_category_table_growth's column: retries from a tiny first table, and none
        growth = gpuutil.synth(4, 0, 200_000, 1 << 20)
        for first in (6, 12, 30):
            call("growth-first-2^%d" % first, (), lambda: build(growth, ["CS_CAT_FIRST_LOG2=%d" % first]))
        call("growth-plain-slots", (), lambda: build(growth, ["CS_CAT_PLAIN_SLOTS"]))
        rnd = random.Random("radix 300")
        small = order.column(order.make_rows(order.random_12_bytes(300, rnd), True, rnd))
        call("radix-300-keys", (), lambda: build(small, ["CS_CAT_RADIX"]))
        # the sampled sizing: the strided k_cat_insert between two over all rows
        call("sampled-4.3M-distinct", (), lambda: build(order.big_distinct_column(False), []))
        for k in (1000, 1 << 20):
            bench = gpuutil.synth(4, 0, 1_000_000, k)
            call("bench-1M-K%d" % k, (), lambda: build(bench, []))
    else:
        import test_gpu_scan_forms as scans

        for name, op, pat, kind, n, switches in scans.CASES:
            call(name, switches, lambda: scan(scans, scans._col(kind, n)[1], op, pat))
        bench = gpuutil.synth(3, 0, 1_000_000)
        for op in (scans.CONTAINS, scans.COUNT):
            for i in range(2):
                call("bench-1M-%s-%d" % (op, i), (), lambda: scan(scans, bench, op, forms.IPV4))


def emit(lines):
    """Prints the dispatches; a run of the runtime's copy / fill kernels becomes one line."""
    run = {}

    def flush():
        if run:
            print("(runtime: %s)" % ", ".join("%d %s" % (n, k) for k, n in sorted(run.items())))
            run.clear()

    for line in lines:
        if line.startswith("__amd_rocclr_"):
            k = line.split()[0][len("__amd_rocclr_"):]
            run[k] = run.get(k, 0) + 1
        else:
            flush()
            print(line)
    flush()


def listing_json(files):
    rows = []
    for f in files:
        with open(f) as fh:
            doc = json.load(fh)
        for tool in doc.get("rocprofiler-sdk-tool", []):
            names = {}
            for k in tool.get("kernel_symbols", []):
                names[k.get("kernel_id")] = k.get("formatted_kernel_name") or k.get("demangled_kernel_name") or k.get("kernel_name")
            for r in tool.get("buffer_records", {}).get("kernel_dispatch", []):
                di = r.get("dispatch_info", {})
                g, w = di.get("grid_size", {}), di.get("workgroup_size", {})
                rows.append((int(r.get("start_timestamp", 0)), int(di.get("dispatch_id", 0)),
                             "%s grid %sx%sx%s wg %sx%sx%s lds %s" % (names.get(di.get("kernel_id"), di.get("kernel_id")), g.get("x"), g.get("y"), g.get("z"),
                                                                     w.get("x"), w.get("y"), w.get("z"), di.get("group_segment_size", "?"))))
    emit(line for _, _, line in sorted(rows))


def listing(d, force_csv=False):
    jfiles = sorted(glob.glob(os.path.join(d, "**", "*results.json"), recursive=True))
    if jfiles and not force_csv:
        return listing_json(jfiles)
    print("# CSV trace: `lds` is LDS_Block_Size, which leaves out the dynamic LDS of a launch")
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit("no *kernel_trace.csv under " + d)
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: (int(r.get("Start_Timestamp", 0)), int(r.get("Dispatch_Id", 0))))
    lines = []
    for r in rows:
        grid = "x".join(r.get(k, "?") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
        wg = "x".join(r.get(k, "?") for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z"))
        lines.append("%s grid %s wg %s lds %s" % (r.get("Kernel_Name", "?"), grid, wg, r.get("LDS_Block_Size", r.get("Group_Segment_Size", "?"))))
    emit(lines)


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run" and sys.argv[2:] in ([], ["replace"], ["scan"], ["split"], ["spans"], ["category"]):
        run(sys.argv[2] if sys.argv[2:] else "replace")
    elif len(sys.argv) >= 3 and sys.argv[1] == "list":
        listing(sys.argv[2], force_csv=sys.argv[3:] == ["csv"])
    else:
        sys.exit(__doc__)
