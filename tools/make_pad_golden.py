"""Writes tests/golden/reference_pad.json and tests/golden/relink_pad_symbols.json: the known answers of the reference's
substring / padding / wrapping tests and the mangled names of the twelve NVStrings members.

The Python tests (python/tests/test_pad.py, test_substr.py, test_wrap.py) are read with `ast`: in every test function the
input list, the call on the instance and the `expected` list are taken in order; where the expectation is a pandas call
(pstrs.str.slice / slice_replace / wrap) it is evaluated here with pandas over the test's parametrize grid.  The C++ tests
(cpp/tests/test_pad.cpp, test_modify.cu) are transcribed below as data, every line checked to hold the case's first
expected literal.  Each case keeps its file:line.

    python3 tools/make_pad_golden.py <reference tree> tests/golden
"""
import ast
import itertools
import json
import os
import sys

PY_TESTS = ["python/tests/test_pad.py", "python/tests/test_substr.py", "python/tests/test_wrap.py"]
OPS = {"get", "repeat", "pad", "ljust", "center", "rjust", "zfill", "wrap", "slice", "slice_from", "slice_replace", "insert"}

PAD_IN = ["12345", "thesé", None, "ARE THE", "tést strings", ""]
MOD_IN = ["Héllo", "thesé", None, "ARE THE", "tést strings", ""]
# (file, line, literal on that line, case): the C++ API (positional arguments of the member)
CPP_CASES = [
    ("cpp/tests/test_pad.cpp", 21, "1234512345", dict(op="repeat", args=[2], input=PAD_IN,
     expected=["1234512345", "theséthesé", None, "ARE THEARE THE", "tést stringstést strings", ""])),
    ("cpp/tests/test_pad.cpp", 15, "tést strings", dict(op="repeat", args=[1], input=PAD_IN, expected=PAD_IN)),
    ("cpp/tests/test_pad.cpp", 35, "12345     ", dict(op="ljust", args=[10], input=PAD_IN,
     expected=["12345     ", "thesé     ", None, "ARE THE   ", "tést strings", "          "])),
    ("cpp/tests/test_pad.cpp", 41, "  12345", dict(op="rjust", args=[7], input=PAD_IN,
     expected=["  12345", "  thesé", None, "ARE THE", "tést strings", "       "])),
    ("cpp/tests/test_pad.cpp", 47, "__12345__", dict(op="center", args=[9, "_"], input=PAD_IN,
     expected=["__12345__", "__thesé__", None, "_ARE THE_", "tést strings", "_________"])),
    ("cpp/tests/test_pad.cpp", 59, "000thesé", dict(op="zfill", args=[8], input=PAD_IN,
     expected=["00012345", "000thesé", None, "0ARE THE", "tést strings", "00000000"])),
    ("cpp/tests/test_pad.cpp", 69, "ARE\\nTHE", dict(op="wrap", args=[3], input=PAD_IN,
     expected=["12345", "thesé", None, "ARE\nTHE", "tést\nstrings", ""])),
    ("cpp/tests/test_modify.cu", 18, "Hé___lo", dict(op="slice_replace", args=["___", 2, 3], input=MOD_IN,
     expected=["Hé___lo", "th___sé", None, "AR___ THE", "té___t strings", "___"])),
    ("cpp/tests/test_modify.cu", 24, "Hél||lo", dict(op="slice_replace", args=["||", 3, 3], input=MOD_IN,
     expected=["Hél||lo", "the||sé", None, "ARE|| THE", "tés||t strings", "||"])),
    ("cpp/tests/test_modify.cu", 30, "Héllox", dict(op="slice_replace", args=["x", -1, -1], input=MOD_IN,
     expected=["Héllox", "theséx", None, "ARE THEx", "tést stringsx", "x"])),
    ("cpp/tests/test_modify.cu", 44, "\"l\"", dict(op="slice", args=[2, 3], input=MOD_IN, expected=["l", "e", None, "E", "s", ""])),
    ("cpp/tests/test_modify.cu", 50, "t strings", dict(op="slice", args=[3, -1], input=MOD_IN,
     expected=["lo", "sé", None, " THE", "t strings", ""])),
    ("cpp/tests/test_modify.cu", 56, "\"H\"", dict(op="get", args=[0], input=MOD_IN, expected=["H", "t", None, "A", "t", ""])),
    ("cpp/tests/test_modify.cu", 69, "\" strings\"", dict(op="slice_from", args=[[4] * 6, None], input=MOD_IN,
     expected=["o", "é", None, "THE", " strings", ""])),
    ("cpp/tests/test_modify.cu", 102, "H***éllo", dict(op="insert", args=["***", 1], input=MOD_IN,
     expected=["H***éllo", "t***hesé", None, "A***RE THE", "t***ést strings", ""])),
    ("cpp/tests/test_modify.cu", 108, "Héllo++", dict(op="insert", args=["++", -1], input=MOD_IN,
     expected=["Héllo++", "thesé++", None, "ARE THE++", "tést strings++", "++"])),
]
SYMBOLS = [
    "_ZN9NVStrings3getEj", "_ZN9NVStrings3padEjNS_7padsideEPKc", "_ZN9NVStrings4wrapEj", "_ZN9NVStrings5ljustEjPKc",
    "_ZN9NVStrings5rjustEjPKc", "_ZN9NVStrings5sliceEiii", "_ZN9NVStrings5zfillEj", "_ZN9NVStrings6centerEjPKc",
    "_ZN9NVStrings6insertEPKci", "_ZN9NVStrings6repeatEj", "_ZN9NVStrings10slice_fromEPKiS1_", "_ZN9NVStrings13slice_replaceEPKcii",
]


def _lit(node, env):
    if isinstance(node, ast.Name):
        return env[node.id]
    if isinstance(node, ast.Call):  # np.asarray([...], dtype=...), rmm.to_device(...), x.device_ctypes_pointer.value
        return _lit(node.args[0], env)
    if isinstance(node, ast.Attribute):
        return _lit(node.value, env)
    return ast.literal_eval(node)


def _grid(fn):
    """the parametrize decorators of a test -> list of {name: value} (every combination)"""
    names, values = [], []
    for d in fn.decorator_list:
        if isinstance(d, ast.Call) and getattr(d.func, "attr", "") == "parametrize":
            names.append(ast.literal_eval(d.args[0]))
            values.append(ast.literal_eval(d.args[1]))
    return [dict(zip(names, combo)) for combo in itertools.product(*values)] or [{}]


def python_cases(ref, path):
    import pandas as pd

    tree = ast.parse(open(os.path.join(ref, path)).read())
    out = []
    for fn in tree.body:
        if not isinstance(fn, ast.FunctionDef) or not fn.name.startswith("test_"):
            continue
        for params in _grid(fn):
            env = dict(params)
            call = None
            for st in fn.body:
                if not isinstance(st, ast.Assign) or not isinstance(st.targets[0], ast.Name):
                    continue
                name, v = st.targets[0].id, st.value
                if name == "index" and isinstance(v, ast.Constant):  # (test_get overrides its own parameter)
                    env[name] = v.value
                elif name == "d_arr":  # (the device array of slice_from: its host values)
                    env["d_arr"] = _lit(v, env)
                elif name == "s" or (isinstance(v, ast.Call) and getattr(v.func, "attr", "") == "to_device"):
                    env["input"] = _lit(v if name == "s" else v.args[0], env)
                    if name == "s":
                        env["s"] = env["input"]
                elif name == "got" and isinstance(v, ast.Call) and getattr(v.func, "attr", "") in OPS:
                    args = [_lit(a, env) for a in v.args]
                    kw = {k.arg: _lit(k.value, env) for k in v.keywords}
                    call = (v.func.attr, args, kw, st.lineno)
                elif name == "expected" and call:
                    op, args, kw, line = call
                    if isinstance(v, ast.Call):  # pandas: pstrs.str.<op>(...)
                        pargs = [_lit(a, env) for a in v.args]
                        res = getattr(pd.Series(env["input"]).str, v.func.attr)(*pargs)
                        expected = [None if (x is None or x != x) else x for x in res.tolist()]
                        origin = "pandas"
                    else:
                        expected = _lit(v, env)
                        origin = "literal"
                    out.append(dict(src="%s:%d" % (path, st.lineno), api="python", op=op, args=args, kwargs=kw,
                                    input=env["input"], expected=expected, expected_from=origin))
    return out


def main(ref, outdir):
    cases = []
    for path, line, needle, case in CPP_CASES:
        text = open(os.path.join(ref, path)).read().splitlines()[line - 1]
        if needle not in text:
            raise SystemExit("%s:%d does not hold %r" % (path, line, needle))
        cases.append(dict(src="%s:%d" % (path, line), api="cpp", kwargs={}, expected_from="literal", **case))
    seen = set()
    for path in PY_TESTS:
        for c in python_cases(ref, path):  # (a parametrize grid repeats values: each case once)
            key = json.dumps([c["src"], c["op"], c["args"], c["kwargs"], c["input"]])
            if key not in seen:
                seen.add(key)
                cases.append(c)
    with open(os.path.join(outdir, "reference_pad.json"), "w") as f:
        json.dump({"about": __doc__.strip().splitlines()[0], "cases": cases}, f, indent=1, ensure_ascii=False)
        f.write("\n")
    with open(os.path.join(outdir, "relink_pad_symbols.json"), "w") as f:
        json.dump({"about": "NVStrings symbols a caller of the twelve substring / padding / wrapping members "
                            "(tests/test_pad_cpu.py CALLER) leaves undefined when compiled against the reference headers",
                   "symbols": sorted(SYMBOLS)}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
