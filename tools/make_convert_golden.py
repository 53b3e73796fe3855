"""Writes tests/golden/reference_convert.json: the inputs and expected outputs of the reference's conversion tests
(python/tests/test_convert.py test_hash ... test_from_booleans, read with `ast`; cpp/tests/test_convert.cu Hash ...
FromIPv4, transcribed below as data), each with its file:line.  Floats are stored as bit patterns in hex (f32 / f64).

    python3 tools/make_convert_golden.py <reference tree> > tests/golden/reference_convert.json
"""
import ast
import json
import math
import struct
import sys


def f32(x):
    return None if x is None else "0x%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def f64(x):
    return None if x is None else "0x%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


NAN32, NAN64, INF32, INF64 = "0x7fc00000", "0x7ff8000000000000", "0x7f800000", "0x7ff0000000000000"


def lit(node):
    """a literal, np.nan / np.inf, or np.array([...], dtype=...) as a plain list"""
    if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "array":
        return lit(node.args[0])
    if isinstance(node, ast.Attribute) and node.attr in ("nan", "inf"):
        return float(node.attr)
    if isinstance(node, ast.List):
        return [lit(e) for e in node.elts]
    return ast.literal_eval(node)


PY_OPS = {"hash": "hash", "stoi": "stoi", "stol": "stol", "stof": "stof", "stod": "stod", "htoi": "htoi", "ip2int": "ip2int",
          "to_booleans": "to_bools", "itos": "itos", "ltos": "ltos", "ftos": "ftos", "dtos": "dtos", "int2ip": "int2ip",
          "from_booleans": "from_bools"}


def python_cases(path, rel):
    tree = ast.parse(open(path).read())
    cases = []
    for fn in tree.body:
        if not isinstance(fn, ast.FunctionDef) or fn.name[5:] not in PY_OPS:
            continue
        env = {}
        for st in fn.body:
            if isinstance(st, ast.Assign):
                name = st.targets[0].id
                v = st.value
                if isinstance(v, ast.Call) and getattr(v.func, "attr", "") == "to_device" and name != "expected":
                    env[name] = ("strings", lit(v.args[0]))
                elif isinstance(v, ast.Call) and isinstance(v.func, ast.Attribute) and v.func.attr in PY_OPS:
                    kw = {k.arg: lit(k.value) for k in v.keywords}
                    op = PY_OPS[v.func.attr]
                    if isinstance(v.func.value, ast.Name) and v.func.value.id == "nvstrings":
                        env["__call"] = dict(op=op, input=env[v.args[0].id][1], kw=kw, line=st.lineno)
                    else:
                        env["__call"] = dict(op=op, input=env[v.func.value.id][1], kw=kw, line=st.lineno)
                elif name == "expected":
                    ex = v
                    if isinstance(ex, ast.Call):
                        ex = ex.args[0]
                    call = env["__call"]
                    case = {"src": "%s:%d" % (rel, call["line"]), "api": "python", "op": call["op"], "input": call["input"],
                            "expected": lit(ex)}
                    for k, val in call["kw"].items():
                        case[k] = val
                    cases.append(case)
                else:
                    try:
                        env[name] = ("values", lit(v))
                    except ValueError:
                        pass
    return cases


def cpp_cases(rel):
    nan = float("nan")
    inf = float("inf")
    c = []

    def add(line, op, inp, exp, **kw):
        d = {"src": "%s:%d" % (rel, line), "api": "cpp", "op": op, "input": inp, "expected": exp}
        d.update(kw)
        c.append(d)

    add(10, "hash", ["thesé", None, "are", "the", "tést", "strings", ""], [126208335, 0, 3771471008, 2967174367, 1378466566, 3184694146, 1257683291])
    ti = ["1234", None, "-876", "543.2", "-0.12", ".55", "-.002", "", "de", "abc123", "123abc", "456e", "-1.78e+5"]
    add(26, "stoi", ti, [1234, 0, -876, 543, 0, 0, 0, 0, 0, 0, 123, 456, -1])
    add(26, "stol", ti, [1234, 0, -876, 543, 0, 0, 0, 0, 0, 0, 123, 456, -1])
    add(56, "itos", [100, 987654321, -12761, 0, 5, -4], ["100", "987654321", "-12761", "0", "5", "-4"])
    add(65, "ltos", [100000, 9876543210, -1276100, 0, 5, -4], ["100000", "9876543210", "-1276100", "0", "5", "-4"])
    add(76, "htoi", ["1234", None, "98BEEF", "1a5", "CAFE", "2face"], [4660, 0, 10010351, 421, 51966, 195278])
    tf = ["1234", None, "-876", "543.2", "-0.12", ".25", "-.002", "", "NaN", "abc123", "123abc", "456e", "-1.78e+5",
          "-122.33644782123456789", "12e+309"]
    add(89, "stof", tf, [1234.0, 0, -876.0, 543.2, -0.12, 0.25, -0.002, 0, nan, 0, 123.0, 456.0, -178000.0, -122.3364486694336, inf])
    add(89, "stod", tf, [1234.0, 0, -876.0, 543.2, -0.12, 0.25, -0.002, 0, nan, 0, 123.0, 456.0, -178000.0, -122.3364478212345, inf])
    add(137, "ftos", [100, 654321.25, -12761.125, 0, 5, -4, nan], ["100.0", "654321.25", "-12761.125", "0.0", "5.0", "-4.0", "NaN"])
    add(146, "dtos", [0.0000012345, 65432125000, -12761.125, 0, 5, -4, inf], ["1.2345e-06", "6.5432125e+10", "-12761.125", "0.0", "5.0", "-4.0", "Inf"])
    add(158, "to_bools", ["false", None, "", "true", "True", "False"], [False, False, False, True, False, False], true="true")
    add(170, "from_bools", [True, False, False, True, True, True], ["true", "false", "false", "true", "true", "true"], true="true", false="false")
    add(182, "ip2int", [None, "", "hello", "41.168.0.1", "127.0.0.1", "41.197.0.1"], [0, 0, 0, 698875905, 2130706433, 700776449])
    add(194, "int2ip", [3232235521, 167772161, 0, 0, 700055553, 700776449], ["192.168.0.1", "10.0.0.1", "0.0.0.0", "0.0.0.0", "41.186.0.1", "41.197.0.1"])
    return c


def encode(case):
    """floats as bit patterns: stof / stod outputs, ftos / dtos inputs"""
    op = case["op"]
    enc = {"stof": f32, "stod": f64}.get(op)
    canon = {"stof": (NAN32, INF32), "stod": (NAN64, INF64)}.get(op)
    if enc:
        out = []
        for v in case["expected"]:
            if v is not None and math.isnan(v):
                out.append(canon[0])
            else:
                out.append(enc(v))
        case["expected"] = out
    if op in ("ftos", "dtos"):
        e = f32 if op == "ftos" else f64
        case["input"] = [e(v) for v in case["input"]]
    if op == "stod" and "-122.33644782" in case["input"]:
        i = case["input"].index("-122.33644782")
        case["deviation"] = {"row": i, "reason": "the reference scales by CUDA's pow(10.0, e), which is not correctly rounded; "
                             "this row is one ulp away from digits * P[e] (convert_ops.h, DESIGN.md Deviations)"}
    return case


def main(ref):
    cases = python_cases(ref + "/python/tests/test_convert.py", "python/tests/test_convert.py")
    cases += cpp_cases("cpp/tests/test_convert.cu")
    json.dump({"about": __doc__.strip().splitlines()[0], "cases": [encode(c) for c in cases]}, sys.stdout, indent=1, ensure_ascii=False)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
