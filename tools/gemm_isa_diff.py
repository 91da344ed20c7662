"""Are two builds of speecht5_amd/csrc/gemm.hip the same device code?  Compares two `hipcc -S --cuda-device-only` outputs (the flags of
tools/epilogue_isa_order.py) kernel by kernel: a kernel's body is everything from its label to its `; Occupancy:` comment, i.e. the
instruction stream AND the resource footer (NumVgprs, NumAgprs, ScratchSize, Occupancy, codeLenInByte).  Compiler-local label numbers
(.LBB<function>_<block>, .Lfunc_end<function>, .Ltmp<n>) depend on what else the file holds and are normalised.  No GPU needed.

Prints the kernels found in one file only, the kernels whose bodies differ (with the first differing line) and the number of identical
ones; exit status 1 on any difference.

usage: gemm_isa_diff.py OLD.s NEW.s"""
import re, sys
from epilogue_isa_order import kernel_bodies, demangle


def normalised(body):
    out = []
    for line in body:
        line = re.sub(r"\bL?BB\d+_(\d+)", r"BB_\1", line)      # (.LBB12_3 labels, and "Header=BB12_3" in the loop comments)
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
        line = re.sub(r"\.Ltmp\d+", ".Ltmp", line)
        out.append(re.sub(r"\s+", " ", line).strip())    # (the comment column moves with the label's width)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = ({k: normalised(b) for k, b in kernel_bodies(p).items()} for p in sys.argv[1:3])
    dem = demangle(sorted(set(old) | set(new)))
    short = lambda n: re.sub(r"\(.*$", "", dem[n].replace("(anonymous namespace)::", "")).replace("void ", "")
    bad = 0
    for tag, a, b in (("only in OLD", old, new), ("only in NEW", new, old)):
        for n in sorted(set(a) - set(b)):
            print(f"{tag}: {short(n)}")
            bad += 1
    same = 0
    for n in sorted(set(old) & set(new)):
        if old[n] == new[n]:
            same += 1
            continue
        bad += 1
        i = next((i for i, (x, y) in enumerate(zip(old[n], new[n])) if x != y), min(len(old[n]), len(new[n])))
        line = lambda b: b[i].strip() if i < len(b) else "<end of body>"
        print(f"DIFFERS: {short(n)}  ({len(old[n])} / {len(new[n])} lines) at body line {i + 1}:\n    old: {line(old[n])}\n    new: {line(new[n])}")
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW: {same} identical, {bad} different or unmatched")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
