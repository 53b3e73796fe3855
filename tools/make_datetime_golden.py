"""Writes tests/golden/reference_datetime.json and tests/golden/relink_datetime_symbols.json: the known answers of the
reference's timestamp tests (cpp/tests/test_datetime.cu ToTimestamp / FromTimestamp, python/tests/test_datetime.py and
the timestamp2int docstring of python/nvstrings.py), transcribed below as data with their file:line -- every line is
checked to hold the case's first literal -- and the mangled names of the two NVStrings members.

    python3 tools/make_datetime_golden.py <reference tree> tests/golden
"""
import json
import os
import sys

DEFAULT = "%Y-%m-%dT%H:%M:%SZ"
# (file, line, literal on that line, case).  Python-test expectations come from pandas there (pd.Timestamp -> int64 ns,
# compared with np.allclose); they are stored here in the test's units.
CASES = [
    ("cpp/tests/test_datetime.cu", 14, "1974-02-28T01:23:45Z",
     dict(api="cpp", op="timestamp2long", format=DEFAULT, units="s",
          input=["1974-02-28T01:23:45Z", "2019-07-17T21:34:37Z", None, ""], expected=[131246625, 1563399277, 0, 0], count=2)),
    ("cpp/tests/test_datetime.cu", 26, "12.28.1982",
     dict(api="cpp", op="timestamp2long", format="%m-%d-%Y", units="D", input=["12.28.1982", "07.17.2019"],
          expected=[4744, 18094], count=2)),
    ("cpp/tests/test_datetime.cu", 40, "1563399273",
     dict(api="cpp", op="long2timestamp", format="%m/%d/%Y %H:%M", units="s", input=[1563399273], expected=["07/17/2019 21:34"])),
    ("cpp/tests/test_datetime.cu", 49, "1563399273123",
     dict(api="cpp", op="long2timestamp", format="%H:%M:%S.%f", units="ms", input=[1563399273123], expected=["21:34:33.123"])),
    ("python/nvstrings.py", 873, "2019-03-20T12:34:56Z",
     dict(api="python", op="timestamp2long", format=None, units="s", input=["2019-03-20T12:34:56Z"], expected=[1553085296], count=1)),
    ("python/tests/test_datetime.py", 11, "2019-03-20T12:34:56Z",
     dict(api="python", op="timestamp2long", format=None, units="s", input=["2019-03-20T12:34:56Z", "2020-02-29T23:59:59Z"],
          expected=[1553085296, 1583020799], count=2)),
    ("python/tests/test_datetime.py", 19, "2019-03-20T12:34:56Z",
     dict(api="python", op="timestamp2long", format=None, units="ms", input=["2019-03-20T12:34:56Z", "2020-02-29T23:59:59Z"],
          expected=[1553085296000, 1583020799000], count=2)),
    ("python/tests/test_datetime.py", 28, "1553085296",
     dict(api="python", op="long2timestamp", format=None, units="s", input=[1553085296, 1582934400],
          expected=["2019-03-20T12:34:56Z", "2020-02-29T00:00:00Z"])),
]
SYMBOLS = ["_ZN9NVStrings14long2timestampEPKmjNS_15timestamp_unitsEPKcPKhb", "_ZN9NVStrings14timestamp2longEPKcNS_15timestamp_unitsEPmb"]


def main(ref, outdir):
    cases = []
    for path, line, needle, case in CASES:
        with open(os.path.join(ref, path)) as f:
            text = f.read().splitlines()[line - 1]
        if needle not in text:
            raise SystemExit("%s:%d does not hold %r" % (path, line, needle))
        cases.append(dict(src="%s:%d" % (path, line), **case))
    with open(os.path.join(outdir, "reference_datetime.json"), "w") as f:
        json.dump({"about": __doc__.strip().splitlines()[0], "cases": cases}, f, indent=1)
        f.write("\n")
    with open(os.path.join(outdir, "relink_datetime_symbols.json"), "w") as f:
        json.dump({"about": "NVStrings symbols a caller of timestamp2long / long2timestamp (tests/test_datetime_cpu.py CALLER) "
                            "leaves undefined when compiled against the reference headers", "symbols": sorted(SYMBOLS)}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
