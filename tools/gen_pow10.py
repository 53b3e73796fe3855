"""Writes the power-of-ten table of custrings_amd/csrc/convert_ops.h: P[e] for e in [-308, 308], the double
nearest to 10^e (Python's float("1e<e>") is correctly rounded), as C++17 hexadecimal floating literals so that
every compiler reads back the same bits.

    python3 tools/gen_pow10.py > /tmp/table.inc   (then paste between the markers in convert_ops.h)
"""


def rows():
    vals = [float("1e%d" % e).hex() for e in range(-308, 309)]
    for i in range(0, len(vals), 4):
        yield "    " + ", ".join(vals[i : i + 4]) + ","


if __name__ == "__main__":
    print("\n".join(rows()))
