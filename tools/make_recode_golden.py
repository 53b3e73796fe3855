"""Writes tests/golden/reference_recode.json and tests/golden/relink_recode_symbols.json: the known answers of the reference's
tests of url_encode / url_decode / translate / fillna / index / rindex, and the mangled names of the five NVStrings members.

The cases are transcribed below as data; every one names its file:line and a literal that line must hold, which is checked
against the reference tree.  Where a Python test's expectation is a pandas or urllib call, it is evaluated here: with pandas
when it can be imported, else with the plain-Python equivalent (str.translate per row, None kept) -- the two agree on these
inputs.  A case: op, input rows, args, expected rows.  translate's table is a list of [code point, code point] pairs in the
caller's order (0: drop); fillna's argument is {"str": ...} or {"column": [...]}.

    python3 tools/make_recode_golden.py <reference tree> tests/golden
"""
import json
import os
import string
import sys
import urllib.parse

MODIFY_IN = ["Héllo", "thesé", None, "ARE THE", "tést strings", ""]
URL_ENC_IN = ["www.nvidia.com/rapids?p=é", "/_file-7.txt", "a b+c~d", "e\tfgh\\jklmnopqrstuvwxyz", "ABCDEFGHIJKLMNOPQRSTUVWXYZ",
              "0123456789", " \t\f\n", None, ""]
URL_DEC_IN = ["www.nvidia.com/rapids/%3Fp%3D%C3%A9", "/_file-1234567890.txt", "a%20b%2Bc~defghijklmnopqrstuvwxyz", "%25-accent%c3%a9d",
              "ABCDEFGHIJKLMNOPQRSTUVWXYZ", "01234567890", None, ""]
# (file, line, literal on that line, case)
CPP_CASES = [
    ("cpp/tests/test_url.cpp", 16, "strs->url_encode()",
     dict(op="url_encode", input=URL_ENC_IN, args=[],
          expected=["www.nvidia.com%2Frapids%3Fp%3D%C3%A9", "%2F_file-7.txt", "a%20b%2Bc~d", "e%09fgh%5Cjklmnopqrstuvwxyz",
                    "ABCDEFGHIJKLMNOPQRSTUVWXYZ", "0123456789", "%20%09%0C%0A", None, ""])),
    ("cpp/tests/test_url.cpp", 34, "strs->url_decode()",
     dict(op="url_decode", input=URL_DEC_IN, args=[],
          expected=["www.nvidia.com/rapids/?p=é", "/_file-1234567890.txt", "a b+c~defghijklmnopqrstuvwxyz", "%-accentéd",
                    "ABCDEFGHIJKLMNOPQRSTUVWXYZ", "01234567890", None, ""])),
    ("cpp/tests/test_modify.cu", 79, 'strs->fillna("||")',
     dict(op="fillna", input=MODIFY_IN, args={"str": "||"}, expected=["Héllo", "thesé", "||", "ARE THE", "tést strings", ""])),
    ("cpp/tests/test_modify.cu", 87, "strs->fillna(*dnas)",
     dict(op="fillna", input=MODIFY_IN, args={"column": ["1", "2", "3", "4", "5", "6"]},
          expected=["Héllo", "thesé", "3", "ARE THE", "tést strings", ""])),
    ("cpp/tests/test_modify.cu", 125, "strs->translate(",
     dict(op="translate", input=MODIFY_IN, args=[[ord("e"), ord("E")], [ord("H"), ord("h")]],
          expected=["héllo", "thEsé", None, "ARE ThE", "tést strings", ""])),
]
CPP_INPUT_LINES = [("cpp/tests/test_modify.cu", 10, "tést strings"), ("cpp/tests/test_url.cpp", 10, "www.nvidia.com/rapids?p=é"),
                   ("cpp/tests/test_url.cpp", 29, "%3Fp%3D%C3%A9")]

URLS1 = ["http://www.hellow.com", "/home/nvidia/nfs", "123.45 ~ABCDEF"]
URLS2 = ["http://www.hellow.com?k1=acc%C3%A9nted&k2=a%2F/b.c", "%2Fhome%2fnfs", "987%20ZYX"]
TR_IN1 = ["hello", "there", "world", "accéntéd", None, ""]
TR_IN2 = ["This, of course, is only an example!", "And; will have @all the #punctuation that $money can buy.",
          "The %percent & the *star along with the (parenthesis) with dashes-and-under_lines.", "Equations: 3+3=6; 3/4 < 1 and > 0"]
TR_TABLES = [("{}", {}), ('str.maketrans("e", "a")', str.maketrans("e", "a")), ('str.maketrans("elh", "ELH")', str.maketrans("elh", "ELH")),
             ('str.maketrans("", "", string.punctuation)', str.maketrans("", "", string.punctuation)),
             ('str.maketrans(string.punctuation, " " * len(string.punctuation))', str.maketrans(string.punctuation, " " * len(string.punctuation)))]
INDEX_IN = ["he-llo", "-there-", "world-", "accént-éd", None, "-"]


def series_translate(rows, table):
    try:
        import pandas as pd
        return [None if v is None or v != v else v for v in pd.Series(rows).str.translate(table).tolist()]
    except ImportError:
        return [None if r is None else r.translate(table) for r in rows]


def series_fillna(rows, repl):
    try:
        import pandas as pd
        return pd.Series(rows).fillna(repl).tolist()
    except ImportError:
        return [repl if r is None else r for r in rows]


def python_cases(line):
    out = []

    def add(path, no, needle, **case):
        if needle not in line(path, no):
            raise SystemExit("%s:%d does not hold %r" % (path, no, needle))
        out.append(dict(src="%s:%d" % (path, no), api="python", **case))

    add("python/tests/test_url.py", 18, "s.url_encode()", op="url_encode", input=URLS1, args=[],
        expected=[urllib.parse.quote(u, safe="~") for u in URLS1])
    add("python/tests/test_url.py", 27, "s.url_decode()", op="url_decode", input=URLS2, args=[],
        expected=[urllib.parse.unquote(u) for u in URLS2])
    # (the list tables pandas cannot take are expected failures there: only the empty list has an expectation)
    add("python/tests/test_translate.py", 62, "strs.translate(table)", op="translate", input=TR_IN1, args=[], expected=series_translate(TR_IN1, {}))
    for text, table in TR_TABLES:
        if text not in " ".join(line("python/tests/test_translate.py", n) for n in range(70, 75)):
            raise SystemExit("python/tests/test_translate.py:70-74 does not hold %r" % text)
        pairs = [[k, 0 if v is None else v] for k, v in table.items()]
        add("python/tests/test_translate.py", 81, "strs.translate(table)", op="translate", input=TR_IN1, args=pairs, table=text,
            expected=series_translate(TR_IN1, table))
        add("python/tests/test_translate.py", 93, "strs.translate(table)", op="translate", input=TR_IN2, args=pairs, table=text,
            expected=series_translate(TR_IN2, table))
    fill_in = ["abcdefghij", "0123456789", "9876543210", None, "accénted", ""]
    add("python/tests/test_substr.py", 72, "strs.fillna(repl)", op="fillna", input=fill_in, args={"str": ""}, expected=series_fillna(fill_in, ""))
    add("python/tests/test_compare.py", 109, 'strs.index("-")', op="index", input=INDEX_IN, args=["-"], expected=[2, 0, 5, 6, None, 0])
    add("python/tests/test_compare.py", 118, 'strs.rindex("-")', op="rindex", input=INDEX_IN, args=["-"], expected=[2, 6, 5, 6, None, 0])
    return out


SYMBOLS = ["_ZN9NVStrings9translateEPSt4pairIjjEj", "_ZN9NVStrings6fillnaEPKc", "_ZN9NVStrings6fillnaERS_", "_ZN9NVStrings10url_encodeEv",
           "_ZN9NVStrings10url_decodeEv"]


def main(ref, outdir):
    def line(path, no):
        return open(os.path.join(ref, path), encoding="utf-8").read().splitlines()[no - 1]

    for path, no, needle in CPP_INPUT_LINES:
        if needle not in line(path, no):
            raise SystemExit("%s:%d does not hold %r" % (path, no, needle))
    cases = []
    for path, no, needle, case in CPP_CASES:
        if needle not in line(path, no):
            raise SystemExit("%s:%d does not hold %r" % (path, no, needle))
        cases.append(dict(src="%s:%d" % (path, no), api="cpp", **case))
    cases += python_cases(line)
    with open(os.path.join(outdir, "reference_recode.json"), "w") as f:
        json.dump({"about": "Known answers of the reference's own tests of url_encode, url_decode, translate, fillna, index and rindex, each case with its file:line", "cases": cases}, f, indent=1, ensure_ascii=False)
        f.write("\n")
    with open(os.path.join(outdir, "relink_recode_symbols.json"), "w") as f:
        json.dump({"about": "NVStrings symbols a caller of translate, the two fillna members, url_encode and url_decode "
                            "(tests/test_recode_cpu.py CALLER) leaves undefined when compiled against the reference headers",
                   "symbols": sorted(SYMBOLS)}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
