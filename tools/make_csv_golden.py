"""Writes the from_csv fixtures under tests/golden: tweets_head.csv (the first 64 lines of the reference's data/tweets.csv),
reference_csv.json (the five expected rows of python/tests/test_memory.py:10-16 for column 7, and the docstring example of
python/nvstrings.py:87-94) and relink_csv_symbols.json (the mangled name of NVStrings::create_from_csv).

The expectations are transcribed below as data; every one names its file:line and is checked against the reference tree.

    python3 tools/make_csv_golden.py <reference tree> tests/golden
"""
import json
import os
import sys

HEAD_LINES = 64
TWEETS = [
    ("python/tests/test_memory.py", 11, "@Bill_Porter nice to know that your site is back :-)"),
    ("python/tests/test_memory.py", 12, "@sudhamshu after trying out various tools to take notes and I found that paper is the best to take notes and to maintain todo lists."),
    ("python/tests/test_memory.py", 13, "@neetashankar Yeah, I got the connection. I am getting 20 mbps for a 15 mbps connection. Customer service is also good."),
    ("python/tests/test_memory.py", 14, '@Bill_Porter All posts from your website http://t.co/NUWn5HUFsK seems to have been deleted. I am getting a ""Not Found"" page even in homepage'),
    ("python/tests/test_memory.py", 15, 'Today is ""bring your kids"" day at office and the entire office is taken over by cute little creatures ;)'),
]
TWEETS_CALL = ("python/tests/test_memory.py", 8, 'nvstrings.from_csv("../../data/tweets.csv", 7)')
DOC_FILE = [("python/nvstrings.py", 88, "header1,header2,header3"), ("python/nvstrings.py", 89, "r1c1,r1c2,r1c3"), ("python/nvstrings.py", 90, "r2c1,r2c2,r2c3")]
DOC_CALL = ("python/nvstrings.py", 92, 'nvstrings.from_csv("file.csv",2)')
DOC_RESULT = ("python/nvstrings.py", 94, "['r1c3','r2c3']")
DECLARATION = ("cpp/include/NVStrings.h", 146, "static NVStrings* create_from_csv( const char* csvfile, unsigned int column, unsigned int lines=0, sorttype stype=none, bool nullIsEmpty=false);")
FLAGS = [("cpp/src/util.h", 27, "#define CSV_SORT_LENGTH    1"), ("cpp/src/util.h", 28, "#define CSV_SORT_NAME      2"), ("cpp/src/util.h", 29, "#define CSV_NULL_IS_EMPTY   8")]
SYMBOL = "_ZN9NVStrings15create_from_csvEPKcjjNS_8sorttypeEb"


def main(ref, outdir):
    def line(path, no):
        return open(os.path.join(ref, path), encoding="utf-8").read().splitlines()[no - 1]

    def holds(path, no, needle):
        if " ".join(needle.split()) not in " ".join(line(path, no).split()):
            raise SystemExit("%s:%d does not hold %r" % (path, no, needle))

    for path, no, text in TWEETS + DOC_FILE + [TWEETS_CALL, DOC_CALL, DOC_RESULT, DECLARATION] + FLAGS:
        holds(path, no, text)
    with open(os.path.join(ref, "data", "tweets.csv"), "rb") as f:
        head = b"".join(f.readlines()[:HEAD_LINES])
    if b"\r" in head or b"\0" in head or b'""' not in head:
        raise SystemExit("data/tweets.csv: the head is not LF-only text with doubled quotes")
    with open(os.path.join(outdir, "tweets_head.csv"), "wb") as f:
        f.write(head)
    cases = [
        dict(src="%s:%d-%d" % (TWEETS[0][0], TWEETS[0][1] - 1, TWEETS[-1][1] + 1), file="tweets_head.csv", column=7, lines=0, flags=0, first=len(TWEETS),
             expected=[t[2] for t in TWEETS]),
        dict(src="%s:%d-%d" % (DOC_FILE[0][0], DOC_FILE[0][1] - 1, DOC_RESULT[1]), text="".join(t[2] + "\n" for t in DOC_FILE), column=2, lines=0, flags=0,
             expected=["r1c3", "r2c3"]),
    ]
    with open(os.path.join(outdir, "reference_csv.json"), "w") as f:
        json.dump({"about": "Known answers of the reference's from_csv: its own test (the first rows of column 7 of data/tweets.csv; `first`: how many rows "
                            "the test looks at) and its docstring example, each with its file:line", "cases": cases}, f, indent=1, ensure_ascii=False)
        f.write("\n")
    with open(os.path.join(outdir, "relink_csv_symbols.json"), "w") as f:
        json.dump({"about": "The NVStrings symbol a caller of create_from_csv (tests/test_csv_cpu.py CALLER) leaves undefined when compiled against the "
                            "reference headers", "symbols": [SYMBOL]}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
