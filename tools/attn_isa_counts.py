"""Static instruction counts of the fused-attention kernels (speecht5_amd/csrc/flash_attn2.hip), per kernel, from `hipcc -S`.

Compiles the file with the flags of tools/barrier_audit.py (= csrc/Makefile plus -S --cuda-device-only), splits the assembly
into kernels and counts the instruction classes the attention work of DESIGN.md section 7 argues with: VALU, v_exp_f32 (one per
score evaluated, all template copies of the element loop included), waits on LDS, branches, exec-mask regions, 64-bit address
multiplies, bf16 conversions, dropout-hash multiplies, and the register / scratch / occupancy lines of the kernel's footer.
No GPU needed.  usage: attn_isa_counts.py [file.hip | file.s]   (default: the product's flash_attn2.hip)"""
import os, re, subprocess, sys, tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-comment", "-Xclang", "-target-feature", "-Xclang",
         "-packed-fp32-ops", "-S", "--cuda-device-only"]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SRC = os.path.join(HERE, "speecht5_amd", "csrc", "flash_attn2.hip")
COUNTED = (("valu", r"v_(?!mfma|accvgpr)"), ("v_exp_f32", r"v_exp_f32"), ("waitcnt_lgkm", r"s_waitcnt\b.*lgkmcnt"), ("cbranch", r"s_cbranch"),
           ("saveexec", r"s_and_saveexec_b64"), ("v_mad_u64_u32", r"v_mad_u64_u32"), ("v_cvt_pk_bf16_f32", r"v_cvt_pk_bf16_f32"),
           ("v_mul_u32_u24", r"v_mul_u32_u24"), ("mfma", r"v_mfma"), ("global_store", r"global_store"), ("buffer_store", r"buffer_store"),
           ("ds_read", r"ds_read"))
FOOTER = (("vgprs", r";\s*NumVgprs:\s*(\d+)"), ("agprs", r";\s*NumAgprs:\s*(\d+)"), ("scratch", r";\s*ScratchSize:\s*(\d+)"),
          ("occupancy", r";\s*Occupancy:\s*(\d+)"), ("sgprs", r";\s*TotalNumSgprs:\s*(\d+)"))


def compile_to_asm(src=DEFAULT_SRC, out=None):
    out = out or os.path.join(tempfile.mkdtemp(), os.path.basename(src)[:-4] + ".s")
    subprocess.run([HIPCC] + FLAGS + ["-o", out, src], check=True, stderr=subprocess.DEVNULL)
    return out


def kernel_counts(asm_path):
    """{mangled kernel name: {class: count, ..., vgprs, scratch, occupancy}} for every .amdhsa kernel of the file"""
    res, name, body = {}, None, []
    lines = open(asm_path, errors="replace").read().split("\n")
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    for line in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in kernels:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        body.append(line)
        if re.match(r"^;\s*Occupancy:", line):   # the resource comments follow .end_amdhsa_kernel; Occupancy is the last one counted here
            c = {k: sum(1 for x in body if re.match(r"^\s*" + pat, x)) for k, pat in COUNTED}
            text = "\n".join(body)
            for k, pat in FOOTER:
                fm = re.search(pat, text)
                c[k] = int(fm.group(1)) if fm else None
            res[name] = c
            name = None
    return res


def demangle(names):
    out = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True).stdout.strip().split("\n")
    return dict(zip(names, out))


def main():
    arg = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_SRC
    asm = arg if arg.endswith(".s") else compile_to_asm(arg)
    counts = kernel_counts(asm)
    dem = demangle(list(counts))
    cols = [k for k, _ in COUNTED] + [k for k, _ in FOOTER]
    print("kernel | " + " | ".join(cols))
    for n, c in counts.items():
        short = re.sub(r"\(.*$", "", dem[n]).replace("void ", "")
        print(short + " | " + " | ".join(str(c[k]) for k in cols))


if __name__ == "__main__":
    main()
