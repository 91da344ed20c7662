"""profiles/gemm_fp64_ratios.txt from the `gemm fp64 pin:` lines that tests/test_gemm_fp64_gpu.py prints, one per tensor and launch:
    python -m pytest tests/test_gemm_fp64_gpu.py -q -s > LOG;  python tools/gemm_fp64_ratios.py LOG profiles/gemm_fp64_ratios.txt
Keeps, per kernel family (the line's family with the epilogue kind taken off) and tensor, the line with the worst ratio.  No GPU."""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import gemm_reference as G  # noqa: E402

log, out = sys.argv[1], sys.argv[2]
pat = re.compile(r"gemm fp64 pin: (.*?) \| (.*?) \| (\w+) \| kernel (\S+) emulation (\S+) ratio (\S+)")
worst, n = {}, 0
summary = ""
for line in open(log):
    m = pat.search(line)
    if m:
        fam, case, nm, ek, ee, r = m.groups()
        toks = fam.split()
        kind = ""
        if toks[-1] in G.KINDS + G.RT_KINDS:
            kind, toks = toks[-1], toks[:-1]
        key = (" ".join(toks), nm)
        n += 1
        if key not in worst or float(r) > worst[key][0]:
            worst[key] = (float(r), float(ek), float(ee), (kind + " " + case).strip())
    elif re.search(r"\d+ passed|\d+ failed", line):
        summary = line.strip().strip("= ")
with open(out, "w") as f:
    f.write(f"# tests/test_gemm_fp64_gpu.py on an MI355X: {summary}.\n")
    f.write("# Derived from the test's printed lines: pytest tests/test_gemm_fp64_gpu.py -q -s > LOG; python tools/gemm_fp64_ratios.py LOG THIS_FILE\n")
    f.write(f"# {n} comparisons; worst (|kernel - fp64| - floor) / max(|emulation - fp64|, ulp / 2) per kernel family and tensor (bar: {G.BAR:g});\n")
    f.write("# kernel / emulation: the worst absolute errors of that case.  A ratio of 0 (fp32 outputs): the whole error lies inside the summation\n")
    f.write("# floor gamma_(K + 17) S, the bound of an fp32 sum in any order; the absolute columns show kernel and emulation side by side\n")
    f.write(f"{'family':38s} {'tensor':6s} {'ratio':>7s} {'kernel':>10s} {'emulation':>10s}  worst case\n")
    for (fam, nm), (r, ek, ee, case) in worst.items():
        f.write(f"{fam:38s} {nm:6s} {r:7.3f} {ek:10.3e} {ee:10.3e}  {case}\n")
print(open(out).read())
