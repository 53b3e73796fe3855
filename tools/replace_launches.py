"""The launches of the replace route, case by case (dev tool): which kernels a replace call starts, on what grid and with
how much dynamic LDS, for every case of tests/test_gpu_replace_forms.py and for bench.py's pattern on a 1M-row generated
column.  Two builds whose listings agree start the same kernels.

    rocprofv3 --kernel-trace --output-format json -d DIR -- python tools/replace_launches.py run 2> DIR/stream_info.txt
    python tools/replace_launches.py list DIR > listing.txt

`run` makes the calls in a fixed order with CS_STREAM_INFO set (the library's own account of every single-pass launch, on
stderr, behind a `case` line); `list` prints the trace's dispatches in order: kernel, grid, workgroup, LDS.  The LDS is
the dispatch packet's group segment size (`dispatch_info.group_segment_size` of the JSON trace: the kernel's static LDS
plus the dynamic LDS of the launch); the CSV trace's `LDS_Block_Size` column shows 0 for a kernel whose LDS is all
dynamic, so a CSV trace is listed only when there is no JSON one, and says so.
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


def run():
    import gpuutil
    import test_gpu_replace_forms as forms

    L = gpuutil.lib()
    L.check(L.lib.cs_config_set(b"CS_STREAM_INFO", b"1"))

    def call(name, g, op, pat, repl, maxrepl, switches):
        sys.stderr.write("case %s\n" % name)
        sys.stderr.flush()
        for v in switches:
            L.check(L.lib.cs_config_set(v.encode(), b"1"))
        try:
            if op == forms.RE:
                g.replace(pat, repl, maxrepl)
            elif op == forms.LIT:
                g.replace(pat, repl, maxrepl, regex=False)
            else:
                g.replace_with_backrefs(pat, repl)
        finally:
            for v in switches:
                L.check(L.lib.cs_config_set(v.encode(), None))
        sys.stderr.write("route %s\n" % L.lib.cs_debug_last_route().decode())

    for name, op, pat, repl, maxrepl, kind, n, switches in forms.CASES:
        call(name, forms._col(kind, n)[1], op, pat, repl, maxrepl, switches)
    g = gpuutil.synth(3, 0, 1_000_000)
    for i in range(2):  # (the second call finds the column's metadata cached)
        call("bench-1M-%d" % i, g, forms.RE, forms.IPV4, "<IP>", -1, ())


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
    for _, _, line in sorted(rows):
        print(line)


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
    for r in rows:
        grid = "x".join(r.get(k, "?") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
        wg = "x".join(r.get(k, "?") for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z"))
        print("%s grid %s wg %s lds %s" % (r.get("Kernel_Name", "?"), grid, wg, r.get("LDS_Block_Size", r.get("Group_Segment_Size", "?"))))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 3 and sys.argv[1] == "list":
        listing(sys.argv[2], force_csv=sys.argv[3:] == ["csv"])
    else:
        sys.exit(__doc__)
