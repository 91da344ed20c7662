"""Relative-position part of the fused attention backward at the benched shapes: the launch sequence of the GEMM path against
st5_relpos_bwd + st5_relpos_dpe_final (csrc/relpos_bwd.hip).

Shapes (B, H, T, nb): 16 x 12 x 512 (text micro-batch) and 8 x 12 x 499 (speech micro-batch), nb = 320, bf16, q / dq column slices of
[B*T, 3*H*64] buffers as at the call site, seeded random operands.

HIP events around `--reps` back-to-back repetitions on one stream, `--rounds` rounds, the arms ALTERNATED inside every round:
    present   NT GEMM (beta = 1) + k-strided fp32-output GEMM + st5_colsum_ws (two kernels) + st5_cast_from_f32
    fused     st5_relpos_bwd + st5_relpos_dpe_final
and, in the same rounds, every launch of either arm alone (the partial-product GEMM's time is not separable in a kernel trace of the
update: it shares its kernel name with the weight gradients).  A repetition re-reads dQ as the previous one left it: the values drift,
the traffic does not.  The last line is the JSON record; the outputs of one call of each arm on the same inputs are compared byte for
byte first.

    python tools/relpos_bwd_timing.py [--reps 50] [--rounds 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import hip  # noqa: E402

HD = 64
ALPHA = HD ** -0.5
SHAPES = {"text_16x12x512": (16, 12, 512, 320), "speech_8x12x499": (8, 12, 499, 320)}


class Case:
    def __init__(self, dev, B, H, T, nb):
        g = torch.Generator().manual_seed(T)
        self.B, self.H, self.T, self.nb, self.ld = B, H, T, nb, 3 * H * HD
        self.dqp = (torch.randn(B * H, T, nb, generator=g) * 0.5).to(torch.bfloat16).to(dev)
        self.qkv = (torch.randn(B * T, self.ld, generator=g) * 1.2).to(torch.bfloat16).to(dev)
        self.dqkv0 = torch.randn(B * T, self.ld, generator=g).to(torch.bfloat16).to(dev)
        self.pe = torch.randn(nb, HD, generator=g).to(torch.bfloat16).to(dev)
        self.pe_t = self.pe.t().contiguous()
        self.dqkv = self.dqkv0.clone()
        self.part = torch.empty(B * H, nb, HD, dtype=torch.float32, device=dev)
        self.g32 = torch.empty(nb, HD, dtype=torch.float32, device=dev)
        self.dpe = torch.empty(nb, HD, dtype=torch.bfloat16, device=dev)
        self.L = hip.lib()
        self.ws = torch.empty(self.L.st5_colsum_ws_bytes(B * H, nb * HD), dtype=torch.uint8, device=dev)
        self.a = hip.operand(self.dqp, nb, zs0=H * T * nb, zs1=T * nb)

    # ---- the present sequence, launch by launch
    def dq_gemm(self):
        c = self
        hip.gemm(c.a, hip.operand(c.pe_t, c.nb), hip.operand(c.dqkv, c.ld, zs0=c.T * c.ld, zs1=HD), c.T, HD, c.nb, hip.BF16,
                 batch=c.B * c.H, zdiv=c.H, alpha=ALPHA, beta=1.0)

    def part_gemm(self):
        c = self
        hip.gemm(c.a, hip.operand(c.qkv, c.ld, zs0=c.T * c.ld, zs1=HD), hip.operand(c.part, HD, zs0=c.H * c.nb * HD, zs1=c.nb * HD),
                 c.nb, HD, c.T, hip.BF16, batch=c.B * c.H, zdiv=c.H, flags=hip.A_KSTRIDED | hip.B_KSTRIDED | hip.OUT_F32, alpha=ALPHA)

    def colsum(self):
        c = self
        n = c.nb * HD
        hip.check(c.L.st5_colsum_ws(c.part.data_ptr(), c.g32.data_ptr(), c.ws.data_ptr(), c.B * c.H, n, n, 1.0, 0, hip.F32, hip.stream()),
                  "st5_colsum_ws")

    def cast(self):
        c = self
        hip.check(c.L.st5_cast_from_f32(c.g32.data_ptr(), c.dpe.data_ptr(), 1, c.nb * HD, 0, hip.BF16, hip.stream()), "st5_cast_from_f32")

    def present(self):
        self.dq_gemm(); self.part_gemm(); self.colsum(); self.cast()

    # ---- the one-pass kernels
    def relpos_bwd(self):
        c = self
        hip.check(c.L.st5_relpos_bwd(c.dqp.data_ptr(), c.qkv.data_ptr(), c.ld, c.pe.data_ptr(), c.dqkv.data_ptr(), c.ld, c.part.data_ptr(),
                                     c.B, c.H, c.T, c.nb, ALPHA, None, hip.BF16, hip.stream()), "st5_relpos_bwd")

    def dpe_final(self):
        c = self
        hip.check(c.L.st5_relpos_dpe_final(c.part.data_ptr(), c.dpe.data_ptr(), c.B * c.H, c.nb * HD, None, hip.BF16, hip.stream()),
                  "st5_relpos_dpe_final")

    def fused(self):
        self.relpos_bwd(); self.dpe_final()

    def bytes_once(self):
        """Every operand counted once: dqp, q, dq read and written, the fp32 partials written and read."""
        c = self
        bh = c.B * c.H
        return bh * c.T * c.nb * 2 + bh * c.T * HD * 2 * 3 + bh * c.nb * HD * 4 * 2


def us_per_call(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) / reps * 1e3, 2)


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    record = dict(tool="relpos_bwd_timing", reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(0), shapes={})
    for name, (B, H, T, nb) in SHAPES.items():
        c = Case(dev, B, H, T, nb)
        c.present()
        ref = (c.dqkv.clone(), c.part.clone(), c.dpe.clone())
        c.dqkv.copy_(c.dqkv0); c.part.zero_(); c.dpe.zero_()
        c.fused()
        torch.cuda.synchronize()
        equal = all(same_bytes(x, y) for x, y in zip(ref, (c.dqkv, c.part, c.dpe)))
        arms = dict(present=c.present, fused=c.fused, dq_gemm=c.dq_gemm, part_gemm=c.part_gemm, colsum=c.colsum, cast=c.cast,
                    relpos_bwd=c.relpos_bwd, dpe_final=c.dpe_final)
        for fn in arms.values():          # warm-up of every arm
            for _ in range(3):
                fn()
        us = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                us[k].append(us_per_call(fn, args.reps))
        med = {k: statistics.median(v) for k, v in us.items()}
        nbytes = c.bytes_once()
        record["shapes"][name] = dict(B=B, H=H, T=T, nb=nb, outputs_byte_identical=equal, us=us, us_median=med, bytes_once=nbytes,
                                      fused_TB_per_s=round(nbytes / med["fused"] * 1e-6, 3),
                                      present_TB_per_s=round(nbytes / med["present"] * 1e-6, 3))
        print(name, "byte-identical" if equal else "OUTPUTS DIFFER", json.dumps(med), flush=True)
    # per update: 12 encoder layers x (text + speech micro-batch)
    record["per_update_ms"] = {arm: round(12 * sum(s["us_median"][arm] for s in record["shapes"].values()) * 1e-3, 3) for arm in ("present", "fused")}
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(record, open(args.json, "w"), indent=1)
    print(json.dumps(record))
    if not all(s["outputs_byte_identical"] for s in record["shapes"].values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
