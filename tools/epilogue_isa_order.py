"""Order of global loads, global stores and vmcnt waits in the epilogues of the MFMA GEMM kernels (speecht5_amd/csrc/gemm.hip), per
kernel, from `hipcc -S`.  No GPU needed.

Loads and stores share one in-order counter on gfx950, so `s_waitcnt vmcnt(N)` retires everything but the newest N memory operations:
a wait for a side-operand load (residual, pre-activation, old C) issued after a row's store also waits for that store to be
acknowledged.  DESIGN.md 4h moves the side-operand loads of the feature-specialised epilogues ahead of the wave tile's first store;
this tool shows it in the compiled code.  For every kernel it takes the instructions after the last MFMA (the epilogue; the phased
256^2 kernels run two 64 x 64 epilogues there), walks them in program order -- the fall-through path, which is the path of a tile
that lies inside M and N -- and replays the counter:

  loads / stores    global_load_* / global_store_* instructions
  waits             s_waitcnt instructions that name vmcnt
  load_waits        waits that retire at least one load
  store_waits       waits that retire at least one STORE (the round trips the epilogue does not need)
  loads_after_store loads issued after the first store
  order             the sequence, run-length coded: L = load, S = store, w = wait retiring loads only, W = wait retiring a store,
                    . = wait retiring nothing
and the footer's register / scratch / occupancy lines and the code size.

usage: epilogue_isa_order.py [gemm.hip | gemm.s] [--all]      (default: the product's gemm.hip; kernels with an MFMA only;
                                                               --all also lists kernels whose epilogue has no load)"""
import os, re, subprocess, sys, tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-comment", "-Xclang", "-target-feature", "-Xclang",
         "-packed-fp32-ops", "-S", "--cuda-device-only"]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SRC = os.path.join(HERE, "speecht5_amd", "csrc", "gemm.hip")
FOOTER = (("vgprs", r";\s*NumVgprs:\s*(\d+)"), ("agprs", r";\s*NumAgprs:\s*(\d+)"), ("scratch", r";\s*ScratchSize:\s*(\d+)"),
          ("occupancy", r";\s*Occupancy:\s*(\d+)"), ("code_bytes", r";\s*codeLenInByte\s*=\s*(\d+)"))


def compile_to_asm(src, out):
    subprocess.run([HIPCC] + FLAGS + ["-o", out, src], check=True, stderr=subprocess.DEVNULL)
    return out


def kernel_bodies(asm_path):
    """{mangled kernel name: [lines from the kernel's label to its Occupancy comment]}"""
    res, name, body = {}, None, []
    text = open(asm_path, errors="replace").read()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    for line in text.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in kernels:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        body.append(line)
        if re.match(r"^;\s*Occupancy:", line):
            res[name] = body
            name = None
    return res


def replay(body):
    """The epilogue's memory events and the counter replay; None for a kernel without an MFMA."""
    ins = [x.strip() for x in body if re.match(r"^\s+[a-z]", x)]
    last = max((i for i, x in enumerate(ins) if x.startswith("v_mfma")), default=None)
    if last is None:
        return None
    pending, seq = [], []          # pending: outstanding operations, oldest first
    c = dict(loads=0, stores=0, waits=0, load_waits=0, store_waits=0, loads_after_store=0)
    tail = ins[last + 1:]
    end = max((i for i, x in enumerate(tail) if x.startswith("global_store") or x.startswith("buffer_store")), default=-1)
    for x in tail[:end + 1]:      # (up to the last store: what the assembler lays out behind it belongs to other paths)
        if x.startswith("global_load") or x.startswith("buffer_load"):
            c["loads"] += 1
            c["loads_after_store"] += 1 if c["stores"] else 0
            pending.append("L"); seq.append("L")
        elif x.startswith("global_store") or x.startswith("buffer_store") or x.startswith("global_atomic"):
            c["stores"] += 1
            pending.append("S"); seq.append("S")
        elif x.startswith("s_waitcnt"):
            m = re.search(r"vmcnt\((\d+)\)", x)
            if not m:
                continue
            keep = int(m.group(1))
            done = pending[:max(0, len(pending) - keep)]
            pending = pending[len(done):]
            c["waits"] += 1
            c["load_waits"] += 1 if "L" in done else 0
            c["store_waits"] += 1 if "S" in done else 0
            seq.append("W" if "S" in done else "w" if "L" in done else ".")
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        out.append(seq[i] + (str(j - i) if j - i > 1 else ""))
        i = j
    c["order"] = " ".join(out)
    return c


def demangle(names):
    # (c++filt does not know the DF16b spelling of __bf16; the vendor-extension spelling demangles to the same text)
    out = subprocess.run(["c++filt"] + [n.replace("DF16b", "u6__bf16") for n in names], capture_output=True, text=True).stdout.strip().split("\n")
    return dict(zip(names, out))


def main():
    args = [a for a in sys.argv[1:] if a != "--all"]
    everything = "--all" in sys.argv[1:]
    arg = args[0] if args else DEFAULT_SRC
    if arg.endswith(".s"):
        bodies = kernel_bodies(arg)
    else:
        with tempfile.TemporaryDirectory() as tmp:      # (the assembly is 30 MB: not left behind)
            bodies = kernel_bodies(compile_to_asm(arg, os.path.join(tmp, os.path.basename(arg)[:-4] + ".s")))
    dem = demangle(list(bodies))
    cols = ["loads", "stores", "waits", "load_waits", "store_waits", "loads_after_store"] + [k for k, _ in FOOTER]
    print("kernel | " + " | ".join(cols) + " | order")
    for n, body in bodies.items():
        c = replay(body)
        if c is None or (not everything and c["loads"] == 0):
            continue
        text = "\n".join(body)
        for k, pat in FOOTER:
            fm = re.search(pat, text)
            c[k] = int(fm.group(1)) if fm else None
        short = re.sub(r"\(.*$", "", dem[n].replace("(anonymous namespace)::", "")).replace("void ", "")
        print(short + " | " + " | ".join(str(c[k]) for k in cols) + " | " + c["order"])


if __name__ == "__main__":
    main()
