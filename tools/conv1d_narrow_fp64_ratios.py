"""profiles/conv1d_narrow_fp64_ratios.txt from the `conv1d-narrow-ratio|` and `conv1d-narrow-plan|` lines that
tests/test_conv1d_narrow_fp64_gpu.py prints:
    python -m pytest -m gpu tests/test_conv1d_narrow_fp64_gpu.py -q -s > LOG;  python tools/conv1d_narrow_fp64_ratios.py LOG profiles/conv1d_narrow_fp64_ratios.txt
Keeps, per kernel and epilogue kind, the line with the worst ratio, and per kernel what the plan query reported (launches, tiles per
block, LDS bytes).  No GPU."""
import re
import sys

log, out = sys.argv[1], sys.argv[2]
worst, plans, n, summary = {}, {}, 0, ""
for line in open(log):
    line = line.strip()
    at = line.find("conv1d-narrow-")          # (pytest -q -s prints a test's progress dot in front of the next test's first line)
    line = line[at:] if at > 0 else line
    if line.startswith("conv1d-narrow-ratio|"):
        _, kernel, kind, r, case = line.split("|")
        n += 1
        key = (kernel, kind)
        if key not in worst or float(r) > worst[key][0]:
            worst[key] = (float(r), case)
    elif line.startswith("conv1d-narrow-plan|"):
        _, kernel, info, case = line.split("|")
        p = plans.setdefault(kernel, dict(n=0, info=set()))
        p["n"] += 1
        p["info"].add(re.sub(r" tile \d+", "", info))
    elif re.search(r"\d+ passed|\d+ failed", line):
        summary = line.strip("= ")
with open(out, "w") as f:
    f.write(f"# tests/test_conv1d_narrow_fp64_gpu.py on an MI355X: {summary}.\n")
    f.write("# Derived from the test's printed lines: pytest -m gpu tests/test_conv1d_narrow_fp64_gpu.py -q -s > LOG; python tools/conv1d_narrow_fp64_ratios.py LOG THIS_FILE\n")
    f.write(f"# {n} comparisons; worst (|kernel - fp64| - summation floor) / max(|emulation - fp64|, bf16 ulp / 2) over the elements of a case\n")
    f.write("# (tests/conv1d_narrow_reference.py, bar: 4), per kernel and epilogue kind.\n")
    f.write(f"{'kernel':34s} {'kind':30s} {'ratio':>7s}  worst case\n")
    for (kernel, kind), (r, case) in sorted(worst.items()):
        f.write(f"{kernel:34s} {kind:30s} {r:7.4f}  {case}\n")
    f.write("#\n# what the plan query (st5_conv1d_narrow_plan; cout1: the grid rule) reported for the launches above\n")
    f.write(f"{'kernel':34s} {'launches':>8s}  tiles per block / LDS bytes seen\n")
    for kernel, p in sorted(plans.items()):
        f.write(f"{kernel:34s} {p['n']:8d}  {'; '.join(sorted(p['info']))}\n")
print(open(out).read())
