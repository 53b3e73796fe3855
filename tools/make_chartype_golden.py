"""Writes tests/golden/reference_chartype.json and tests/golden/relink_chartype_symbols.json: the known answers of the reference's
tests of the character-type predicates and of swapcase / capitalize / title, and the mangled names of the twelve NVStrings members.

The Python tests (python/tests/test_case.py, test_convert.py, test_allnulls.py) are read with `ast`: in every test function the
list handed to to_device, the member called on the instance and the `expected` list are taken; test_allnulls is a parametrize
grid over member names with a literal expectation.  The C++ tests (cpp/tests/test_attrs.cu, test_case.cpp) are transcribed below
as data, every line checked to hold the literal the case names.  Each case keeps its file:line.

    python3 tools/make_chartype_golden.py <reference tree> tests/golden
"""
import ast
import json
import os
import sys

OPS = ["isalnum", "isalpha", "isdigit", "isspace", "isdecimal", "isnumeric", "islower", "isupper", "is_empty", "swapcase", "capitalize",
       "title"]
T, F = True, False
ATTRS_IN = ["Héllo", "thesé", None, "ARE THE", "tést strings", "", "1.75", "-34", "+9.8", "17¼", "x³", "2³", " 12⅝", "1234567890", "de",
            "\t\r\n\f "]
CASE_IN = ["Examples aBc", "thesé", None, "ARE THE", "tést strings", ""]
# (file, line of the member call, literal on that line, case)
CPP_CASES = [
    ("cpp/tests/test_attrs.cu", 45, "strs->isalnum(", dict(op="isalnum", expected=[T, T, F, F, F, F, F, F, F, T, T, T, F, T, T, F])),
    ("cpp/tests/test_attrs.cu", 54, "strs->isalpha(", dict(op="isalpha", expected=[T, T, F, F, F, F, F, F, F, F, F, F, F, F, T, F])),
    ("cpp/tests/test_attrs.cu", 63, "strs->isspace(", dict(op="isspace", expected=[F, F, F, F, F, F, F, F, F, F, F, F, F, F, F, T])),
    ("cpp/tests/test_attrs.cu", 80, "strs->isdigit(", dict(op="isdigit", expected=[F, F, F, F, F, F, F, F, F, F, F, T, F, T, F, F])),
    ("cpp/tests/test_attrs.cu", 89, "strs->isdecimal(", dict(op="isdecimal", expected=[F, F, F, F, F, F, F, F, F, F, F, F, F, T, F, F])),
    ("cpp/tests/test_attrs.cu", 98, "strs->isnumeric(", dict(op="isnumeric", expected=[F, F, F, F, F, F, F, F, F, T, F, T, F, T, F, F])),
    ("cpp/tests/test_attrs.cu", 116, "strs->isspace(", dict(op="isspace", expected=[F, F, F, F, F, F, F, F, F, F, F, F, F, F, F, T])),
    ("cpp/tests/test_attrs.cu", 125, "strs->is_empty(", dict(op="is_empty", expected=[F, F, T, F, F, T, F, F, F, F, F, F, F, F, F, F])),
    ("cpp/tests/test_attrs.cu", 142, "strs->isupper(", dict(op="isupper", expected=[F, F, F, T, F, F, T, T, T, T, F, T, T, T, F, T])),
    ("cpp/tests/test_attrs.cu", 151, "strs->islower(", dict(op="islower", expected=[F, T, F, F, T, F, T, T, T, T, T, T, T, T, T, T])),
    ("cpp/tests/test_case.cpp", 34, "eXAMPLES AbC", dict(op="swapcase", expected=["eXAMPLES AbC", "THESÉ", None, "are the", "TÉST STRINGS", ""])),
    ("cpp/tests/test_case.cpp", 44, "Examples abc", dict(op="capitalize", expected=["Examples abc", "Thesé", None, "Are the", "Tést strings", ""])),
    ("cpp/tests/test_case.cpp", 54, "Examples Abc", dict(op="title", expected=["Examples Abc", "Thesé", None, "Are The", "Tést Strings", ""])),
]
CPP_INPUT_LINES = [("cpp/tests/test_attrs.cu", 9, "17¼", ATTRS_IN), ("cpp/tests/test_case.cpp", 8, "Examples aBc", CASE_IN)]
PY_TESTS = ["python/tests/test_case.py", "python/tests/test_convert.py"]
SYMBOLS = ["_ZN9NVStrings7isalnumEPbb", "_ZN9NVStrings7isalphaEPbb", "_ZN9NVStrings7isdigitEPbb", "_ZN9NVStrings7isspaceEPbb",
           "_ZN9NVStrings9isdecimalEPbb", "_ZN9NVStrings9isnumericEPbb", "_ZN9NVStrings7islowerEPbb", "_ZN9NVStrings7isupperEPbb",
           "_ZN9NVStrings8is_emptyEPbb", "_ZN9NVStrings8swapcaseEv", "_ZN9NVStrings10capitalizeEv", "_ZN9NVStrings5titleEv"]


def python_cases(ref, path):
    tree = ast.parse(open(os.path.join(ref, path)).read())
    out = []
    for fn in tree.body:
        if not isinstance(fn, ast.FunctionDef) or not fn.name.startswith("test_"):
            continue
        rows, call = None, None
        for st in fn.body:
            if not isinstance(st, ast.Assign) or not isinstance(st.targets[0], ast.Name):
                continue
            name, v = st.targets[0].id, st.value
            if isinstance(v, ast.Call) and getattr(v.func, "attr", "") == "to_device":
                rows = ast.literal_eval(v.args[0])
            elif name == "got" and isinstance(v, ast.Call) and getattr(v.func, "attr", "") in OPS and not v.args and not v.keywords:
                call = v.func.attr
            elif name == "expected" and call and rows is not None:
                out.append(dict(src="%s:%d" % (path, st.lineno), api="python", op=call, input=rows, expected=ast.literal_eval(v)))
                call = None
    return out


def allnulls_cases(ref):
    path = "python/tests/test_allnulls.py"
    tree = ast.parse(open(os.path.join(ref, path)).read())
    out = []
    for fn in tree.body:
        if not isinstance(fn, ast.FunctionDef) or fn.name != "test_allnulls":
            continue
        funcs = []
        for d in fn.decorator_list:
            if isinstance(d, ast.Call) and getattr(d.func, "attr", "") == "parametrize":
                funcs = ast.literal_eval(d.args[1])
        rows = expected = None
        for st in ast.walk(fn):
            if isinstance(st, ast.Call) and getattr(st.func, "attr", "") == "to_device":
                rows = ast.literal_eval(st.args[0])
            if isinstance(st, ast.Compare) and isinstance(st.comparators[0], ast.List):
                expected = ast.literal_eval(st.comparators[0])
        for f in funcs:
            if f in OPS:
                out.append(dict(src="%s:%d" % (path, fn.lineno), api="python", op=f, input=rows, expected=expected))
    return out


def main(ref, outdir):
    def line(path, no):
        return open(os.path.join(ref, path), encoding="utf-8").read().splitlines()[no - 1]

    for path, no, needle, _ in CPP_INPUT_LINES:
        if needle not in line(path, no):
            raise SystemExit("%s:%d does not hold %r" % (path, no, needle))
    cases = []
    for path, no, needle, case in CPP_CASES:
        if needle not in line(path, no):
            raise SystemExit("%s:%d does not hold %r" % (path, no, needle))
        cases.append(dict(src="%s:%d" % (path, no), api="cpp", input=ATTRS_IN if path.endswith("test_attrs.cu") else CASE_IN, **case))
    for path in PY_TESTS:
        cases += python_cases(ref, path)
    cases += allnulls_cases(ref)
    with open(os.path.join(outdir, "reference_chartype.json"), "w") as f:
        json.dump({"about": __doc__.strip().splitlines()[0], "cases": cases}, f, indent=1, ensure_ascii=False)
        f.write("\n")
    with open(os.path.join(outdir, "relink_chartype_symbols.json"), "w") as f:
        json.dump({"about": "NVStrings symbols a caller of the nine character-type predicates and of swapcase / capitalize / title "
                            "(tests/test_chartype_cpu.py CALLER) leaves undefined when compiled against the reference headers",
                   "symbols": sorted(SYMBOLS)}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
