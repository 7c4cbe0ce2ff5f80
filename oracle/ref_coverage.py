"""oracle/ref_coverage.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Line coverage of the reference's covariance sources under tests/reference_cases.py (`make -C oracle ref-cov`).

    python ref_coverage.py <dir with the instrumented libcocons_ref.so and ref_wrap.gcno>

Runs the case matrix once in a child process on the instrumented library (the counters are written when that
process ends), then asks gcov for its JSON summary and prints, per function of the three reference files, the
number of executable lines, how many ran, and the numbers of those that did not.  Only line numbers and counts are
read or printed: no listing of the sources is produced.  Exit status 1 if an executable line never ran.
"""
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_FILES = ("cocons_full.cpp", "cocons_taper.cpp", "cocons_types.h")

RUN_CASES = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import reference_cases as rc
from oracle import reference
ref = reference.Reference(%(lib)r)
for case in rc.CASES:
    rc.run(case, ref)
print("ran %%d cases on %%s" %% (len(rc.CASES), %(lib)r))
"""


def main(covdir):
    covdir = os.path.abspath(covdir)
    lib = os.path.join(covdir, "libcocons_ref.so")
    code = RUN_CASES % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), lib=lib)
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)
    out = subprocess.check_output(["gcov", "--json-format", "--stdout", "--demangled-names", "-o", covdir, "ref_wrap.cpp"],
                                  cwd=HERE)
    if out[:2] == b"\x1f\x8b":
        out = gzip.decompress(out)
    per = {}        # (file, function) -> {line: count}
    for doc in (json.loads(l) for l in out.decode().splitlines() if l.strip().startswith("{")):
        for f in doc["files"]:
            base = os.path.basename(f["file"])
            if base not in REF_FILES:
                continue
            names = {fn["name"]: fn.get("demangled_name", fn["name"]) for fn in f.get("functions", [])}
            for ln in f["lines"]:
                fn = names.get(ln.get("function_name"), ln.get("function_name") or "?").split("(")[0]
                d = per.setdefault((base, fn), {})
                d[ln["line_number"]] = d.get(ln["line_number"], 0) + ln["count"]
    missed = 0
    print("%-18s %-28s %6s %6s  %s" % ("file", "function", "lines", "ran", "never ran (line numbers)"))
    for (base, fn), d in sorted(per.items()):
        never = sorted(l for l, c in d.items() if c == 0)
        missed += len(never)
        print("%-18s %-28s %6d %6d  %s" % (base, fn, len(d), len(d) - len(never), " ".join(map(str, never)) or "-"))
    print("executable lines: %d, never ran: %d" % (sum(len(d) for d in per.values()), missed))
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "_ref", "cov")))
