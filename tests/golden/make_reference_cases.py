"""Writes tests/golden/reference_<entry>.json: the inputs of tests/reference_cases.py and what the reference's
own compiled code (oracle/_ref/libcocons_ref.so, oracle/Makefile target `ref`) returns for them.

    python tests/golden/make_reference_cases.py

Outputs are kept with 17 significant digits (they parse back to the same doubles), lower triangles only where
the output is symmetric.  "libm" records a few values of the C library's pow / tgamma / exp / cos / sin / log on
the machine that wrote the file: where they are the same bits, tests/test_reference_pin.py holds the live library
to the file bit for bit, elsewhere within the entrywise bound."""
import ctypes
import ctypes.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

import reference_cases as rc  # noqa: E402


def fixture_path(entry):
    return os.path.join(HERE, "reference_%s.json" % entry)


def libm_fingerprint():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    vals = []
    for name, args in (("pow", (703.3, 1.37)), ("pow", (2.0, -0.37)), ("pow", (0.3, 0.5)), ("tgamma", (1.37,)),
                       ("tgamma", (0.61,)), ("exp", (-703.3,)), ("exp", (0.8125,)), ("cos", (1.1,)), ("sin", (2.3,)),
                       ("log", (1.7,))):
        f = getattr(m, name)
        f.restype = ctypes.c_double
        f.argtypes = [ctypes.c_double] * len(args)
        vals.append(float(f(*args)).hex())
    return vals


def num(v):
    """inputs: finite values as JSON numbers (short, exact on the binary grid), the others as strings"""
    v = float(v)
    return v if np.isfinite(v) else repr(v)


def encode_case(case, out):
    d = {}
    for k, v in case.items():
        if k == "theta":
            d[k] = {a: [num(x) for x in vs] for a, vs in v.items()}
        elif k in ("locs", "X", "locs_pred", "X_pred"):
            d[k] = [[num(x) for x in row] for row in v]
        elif k in ("limits", "x"):
            d[k] = [num(x) for x in v]
        else:
            d[k] = v
    d["out"] = [_text(x) for x in rc.stored(case, out)]
    return d


def _text(x):
    """17 significant digits; the sign of a NaN is kept as "-nan" (the % operator drops it)"""
    return ("-nan" if np.signbit(x) else "nan") if np.isnan(x) else "%.17g" % x


def _value(s):
    """float(s), with the sign of "-nan" kept (float() drops it)"""
    return -float("nan") if s == "-nan" else float(s)


def decode_case(d):
    """(case as tests/reference_cases.py writes it, recorded output as float64)"""
    case = {}
    for k, v in d.items():
        if k == "out":
            continue
        if k == "theta":
            case[k] = {a: [float(x) for x in vs] for a, vs in v.items()}
        elif k in ("locs", "X", "locs_pred", "X_pred"):
            case[k] = [[float(x) for x in row] for row in v]
        elif k in ("limits", "x"):
            case[k] = [float(x) for x in v]
        else:
            case[k] = v
    return case, np.array([_value(x) for x in d["out"]], dtype=np.float64)


def load(entry):
    with open(fixture_path(entry)) as f:
        g = json.load(f)
    return g, [decode_case(d) for d in g["cases"]]


def main():
    from oracle import reference
    ref = reference.Reference()
    for entry in rc.ENTRIES:
        cases = rc.by_entry(entry)
        head = {"entry": entry,
                "source": "oracle/_ref/libcocons_ref.so: the reference's compiled code, K_nu from the oracle",
                "libm": libm_fingerprint()}
        lines = [json.dumps(encode_case(c, rc.run(c, ref)), separators=(",", ":")) for c in cases]
        with open(fixture_path(entry), "w") as f:       # one case per line
            f.write(json.dumps(head, separators=(",", ":"))[:-1] + ',"cases":[\n' + ",\n".join(lines) + "\n]}\n")
        print("%s: %d cases, %d bytes" % (os.path.basename(fixture_path(entry)), len(cases),
                                          os.path.getsize(fixture_path(entry))))


if __name__ == "__main__":
    main()
