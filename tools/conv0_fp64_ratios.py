"""profiles/conv0_fp64_ratios.txt from the `conv0-ratio|` and `conv0-split|` lines that tests/test_conv0_fp64_gpu.py prints:
    python -m pytest -m gpu tests/test_conv0_fp64_gpu.py -q -s > LOG;  python tools/conv0_fp64_ratios.py LOG profiles/conv0_fp64_ratios.txt
Keeps, per waveform family (clip pair for the gradients, which sum over clips), form and tensor, the line with the worst ratio, and per
family the case where the matrix-core forward's split-operand bound stands highest above one bf16 ulp of the output.  No GPU."""
import re
import sys

log, out = sys.argv[1], sys.argv[2]
worst, split, n, summary = {}, {}, 0, ""
for line in open(log):
    line = line.strip()
    if line.startswith("conv0-ratio|"):
        _, fam, form, tensor, r, case = line.split("|")
        n += 1
        key = (fam, form, tensor)
        if key not in worst or float(r) > worst[key][0]:
            worst[key] = (float(r), case)
    elif line.startswith("conv0-split|"):
        parts = line.split("|")
        fam, wide, err, shift, case = parts[1], parts[2], parts[3], " ".join(parts[4:-1]), parts[-1]
        v = float(wide.split()[-1])
        if fam not in split or v > split[fam][0]:
            split[fam] = (v, float(err.split()[-1]), float(shift.split()[-1]), case)
    elif re.search(r"\d+ passed|\d+ failed", line):
        summary = line.strip("= ")
order = {"mean": 0, "rstd": 1, "rstd eps-dominated": 2, "out": 3, "dW": 4, "dgamma": 5, "dbeta": 6}
with open(out, "w") as f:
    f.write(f"# tests/test_conv0_fp64_gpu.py on an MI355X: {summary}.\n")
    f.write("# Derived from the test's printed lines: pytest -m gpu tests/test_conv0_fp64_gpu.py -q -s > LOG; python tools/conv0_fp64_ratios.py LOG THIS_FILE\n")
    f.write(f"# {n} comparisons; worst |kernel - fp64| / derived allowance (tests/conv0_reference.py, bar: 1) per waveform family, form and tensor.\n")
    f.write("# mean / rstd: the saved statistics in their allowance (rstd: position in its interval, 1 at either end; eps-dominated pairs have an\n")
    f.write("# interval one fp32 ulp wide on either side); out: every output element; dW / dgamma / dbeta: accumulated onto non-zero seeds, per clip pair\n")
    f.write(f"{'family':16s} {'form':20s} {'tensor':19s} {'ratio':>7s}  worst case\n")
    for (fam, form, tensor), (r, case) in sorted(worst.items(), key=lambda kv: (order[kv[0][2]], kv[0][1], kv[0][0])):
        f.write(f"{fam:16s} {form:20s} {tensor:19s} {r:7.4f}  {case}\n")
    f.write("#\n# matrix-core forward (bf16): the split-operand bound against one bf16 ulp (2^-8 |out|) of the output, outside the eps-dominated\n")
    f.write("# pairs: median over the clip's elements of bound / ulp and of |kernel - fp64| / ulp, and the largest |mean| rstd of the clip\n")
    f.write(f"{'family':16s} {'bound / ulp':>11s} {'error / ulp':>11s} {'|mean| rstd':>11s}  case\n")
    for fam, (v, e, s, case) in sorted(split.items()):
        f.write(f"{fam:16s} {v:11.2f} {e:11.3f} {s:11.1f}  {case}\n")
print(open(out).read())
