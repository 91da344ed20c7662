"""profiles/elementwise_fp64_ratios.txt from the `elementwise fp64 pin:` lines that tests/test_elementwise_fp64_gpu.py prints, one per
class-C tensor and launch:
    python -m pytest tests/test_elementwise_fp64_gpu.py -q -s > LOG;  python tools/elementwise_fp64_ratios.py LOG profiles/elementwise_fp64_ratios.txt
Keeps, per case family, tensor and dtype, the line with the worst ratio (format of profiles/norm_fp64_ratios.txt).  No GPU."""
import re
import sys

log, out = sys.argv[1], sys.argv[2]
pat = re.compile(r"elementwise fp64 pin: (.*?) \| (.*?) \| (.*?) \| kernel (\S+) emulation (\S+) ratio (\S+)")
worst, n, summary = {}, 0, "?"
for line in open(log):
    m = pat.search(line)
    if m:
        fam, case, nm, ek, ee, r = m.groups()
        n += 1
        key = (fam, nm, "bf16" if "bf16" in case else "fp32")
        if key not in worst or float(r) > worst[key][0]:
            worst[key] = (float(r), float(ek), float(ee), case)
    elif re.search(r"\d+ (passed|failed).* in [\d.]+s", line):
        summary = line.strip().strip("= ")
with open(out, "w") as f:
    f.write(f"# tests/test_elementwise_fp64_gpu.py on an MI355X: {summary}.\n")
    f.write(f"# {n} class-C comparisons; worst kernel / emulation ratio per case family, tensor and dtype (bar: 4)\n")
    f.write(f"{'family':<26} {'tensor':<10} {'dtype':<6} {'ratio':>6} {'kernel':>10} {'emulation':>10}  worst case\n")
    for (fam, nm, dt), (r, ek, ee, case) in worst.items():
        f.write(f"{fam:<26} {nm:<10} {dt:<6} {r:6.3f} {ek:10.3e} {ee:10.3e}  {case}\n")
print(open(out).read())
