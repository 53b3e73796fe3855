"""Writes tests/golden/reference_text.json and tests/golden/relink_text_symbols.json: the known answers of the reference's tests of
contains_strings / strings_counts / edit_distance / porter_stemmer_measure / scatter_count, and the mangled names of the six NVText members.

The cases of cpp/tests/test_text.cu and python/tests/test_text.py are transcribed below as data; every case names the line that
holds its expectation and a literal that must be on that line, and the inputs' lines are checked the same way.  Each case keeps
its file:line.  The symbols are what a caller of the six members leaves undefined when compiled against the reference headers.

    python3 tools/make_text_golden.py <reference tree> tests/golden
"""
import json
import os
import subprocess
import sys
import tempfile

T, F = True, False
CPP, PY = "cpp/tests/test_text.cu", "python/tests/test_text.py"
TSTRS = ["the fox jumped over the dog", "the dog chased the cat", "the cat chased the mouse", None, "", "the mouse ate the cheese"]
EDIT_IN = ["dog", None, "cat", "mouse", "pup", "", "puppy"]
PY_IN = ["apples are green", "apples are a fruit", None, ""]
PY_EDIT_IN = ["my favorite sentence", "kittin", "nvidia"]
PY_SCATTER_IN = ["Dickens", "Einstein", "Christie"]
# (file, line, literal on that line)
INPUT_LINES = [(CPP, 9, "the fox jumped over the dog"), (CPP, 13, "the mouse ate the cheese"), (CPP, 55, '"the", "cat"'), (CPP, 72, '"cat ", "dog "'),
               (CPP, 105, '"dog", nullptr, "cat", "mouse"'), (CPP, 110, '"puppy"'), (CPP, 116, '"hog", "not", "cake", "house"'),
               (CPP, 152, '"abandon", nullptr, "abbey", "cleans"'), (CPP, 168, '"Larry", "Curly", "Moe"'), (CPP, 170, "3,0,1"),
               (PY, 102, '"apples are green", "apples are a fruit", None, ""'), (PY, 105, '"apple", "fruit"'), (PY, 124, '"apples are green"'),
               (PY, 127, '"pl", "re"'), (PY, 213, '"my favorite sentence", "kittin", "nvidia"'), (PY, 214, '"kitten"'),
               (PY, 220, '"my least favorite sentence", "fish", "software"'), (PY, 262, '"Dickens", "Einstein", "Christie"'),
               (PY, 272, "[1, 2, 3]"), (PY, 277, "[2, 0, None]")]
# (file, line of the expectation, literal on that line, case)
CASES = [
    (CPP, 61, "true, false, true, true, true, true, false, false, false, false, true, false",
     dict(op="contains_strings", input=TSTRS, targets=["the", "cat"], expected=[[T, F], [T, T], [T, T], [F, F], [F, F], [T, F]])),
    (CPP, 78, "0,0, 0,1, 1,0, 0,0, 0,0, 0,0",
     dict(op="strings_counts", input=TSTRS, targets=["cat ", "dog "], expected=[[0, 0], [0, 1], [1, 0], [0, 0], [0, 0], [0, 0]])),
    (CPP, 111, "5,5,5,5,2,5,0", dict(op="edit_distance", input=EDIT_IN, targets="puppy", expected=[5, 5, 5, 5, 2, 5, 0])),
    (CPP, 120, "1,3,2,1,3,0,0",
     dict(op="edit_distance_column", input=EDIT_IN, targets=["hog", "not", "cake", "house", "fox", None, "puppy"], expected=[1, 3, 2, 1, 3, 0, 0])),
    (CPP, 158, "3, 0, 2, 1, 1, 0, 1",
     dict(op="porter_stemmer_measure", input=["abandon", None, "abbey", "cleans", "trouble", "", "yearly"], expected=[3, 0, 2, 1, 1, 0, 1])),
    (CPP, 176, '"Larry", "Larry", "Larry", "Moe"',
     dict(op="scatter_count", input=["Larry", "Curly", "Moe"], counts=[3, 0, 1], expected=["Larry", "Larry", "Larry", "Moe"])),
    (PY, 109, "[[True, False], [True, True], [False, False], [False, False]]",
     dict(op="contains_strings", input=PY_IN, targets=["apple", "fruit"], expected=[[T, F], [T, T], [F, F], [F, F]])),
    (PY, 131, "[[1, 2], [1, 1], [0, 0], [0, 0]]", dict(op="strings_counts", input=PY_IN, targets=["pl", "re"], expected=[[1, 2], [1, 1], [0, 0], [0, 0]])),
    (PY, 215, "[15, 1, 6]", dict(op="edit_distance", input=PY_EDIT_IN, targets="kitten", expected=[15, 1, 6])),
    (PY, 223, "[6, 5, 7]",
     dict(op="edit_distance_column", input=PY_EDIT_IN, targets=["my least favorite sentence", "fish", "software"], expected=[6, 5, 7])),
    (PY, 270, '"Christie",', dict(op="scatter_count", input=PY_SCATTER_IN, counts=[1, 2, 3],
                                  expected=["Dickens", "Einstein", "Einstein", "Christie", "Christie", "Christie"])),
    (PY, 276, '["Dickens", "Dickens"]', dict(op="scatter_count", input=PY_SCATTER_IN, counts=[2, 0, None], expected=["Dickens", "Dickens"])),
]
CALLER = r"""
#include "NVStrings.h"
#include "NVText.h"
void calls(NVStrings& a, NVStrings& b, bool* f, unsigned int* u) {
  NVText::contains_strings(a, b, f); NVText::strings_counts(a, b, u);
  NVText::edit_distance(NVText::levenshtein, a, "x", u); NVText::edit_distance(NVText::levenshtein, a, b, u);
  NVText::porter_stemmer_measure(a, nullptr, nullptr, u); NVText::scatter_count(a, u);
}
"""


def caller_symbols(include_dir):
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "caller.cpp"), os.path.join(d, "caller.o")
        with open(src, "w") as f:
            f.write(CALLER)
        subprocess.run(["g++", "-std=c++14", "-c", "-I", include_dir, src, "-o", obj], check=True)
        out = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
        return sorted({ln.split()[-1] for ln in out.splitlines() if "NVText" in ln})


def main(ref, outdir):
    def line(path, no):
        return open(os.path.join(ref, path), encoding="utf-8").read().splitlines()[no - 1]

    for path, no, needle in INPUT_LINES:
        if needle not in line(path, no):
            raise SystemExit("%s:%d does not hold %r" % (path, no, needle))
    cases = []
    for path, no, needle, case in CASES:
        if needle not in line(path, no):
            raise SystemExit("%s:%d does not hold %r" % (path, no, needle))
        cases.append(dict(src="%s:%d" % (path, no), api="cpp" if path == CPP else "python", **case))
    with open(os.path.join(outdir, "reference_text.json"), "w") as f:
        json.dump({"about": __doc__.strip().splitlines()[0], "cases": cases}, f, indent=1, ensure_ascii=False)
        f.write("\n")
    symbols = caller_symbols(os.path.join(ref, "cpp", "include"))
    if len(symbols) != 6:
        raise SystemExit("expected six NVText symbols, got %r" % symbols)
    with open(os.path.join(outdir, "relink_text_symbols.json"), "w") as f:
        json.dump({"about": "NVText symbols a caller of contains_strings / strings_counts / both edit_distance overloads / "
                            "porter_stemmer_measure / scatter_count (tools/make_text_golden.py CALLER) leaves undefined when compiled "
                            "against the reference headers",
                   "symbols": symbols}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
