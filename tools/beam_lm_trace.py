"""The per-kernel split of one device-stepped beam search step with the shallow-fusion LM, from a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/beam_lm_trace.py
        one decode="device" call after a warm-up call: Base ASR model and the transformer_lm_t5 preset LM of tools/beam_lm_timing.py,
        1 sentence x beam 5, 41 steps, bf16, lm_weight 0.3, no CTC (no counters in the same run);
    python tools/beam_lm_trace.py --split OUT/<host>/<pid>_kernel_trace.csv
        the second call's steps cut at the launches that open and close them (the decoder's st5_beam_embed_step, the LM's, the fuse,
        the reorder): per step the medians of the LM's skinny GEMM kernels, their combine kernels, the LM's other kernels, the decoder's
        share, the tail, and the LM's GEMM bytes per second (every LM weight is streamed once per step)."""
import argparse
import csv
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def decode():
    import torch
    from beam_lm_timing import build_lm, generator
    from beam_slots_timing import SECONDS, build_model
    from speech_rows_timing import RATE, batch
    dev = torch.device("cuda:0")
    model, d = build_model(dev, torch.bfloat16)
    lm = build_lm(dev, len(d))
    wav, pad = batch([SECONDS * RATE], dev, seed=7)
    sample = {"net_input": {"source": wav, "padding_mask": pad}}
    with torch.no_grad():
        g = generator(model, lm, d, "device", 5, 40, 0.25, False)
        for _ in range(2):
            g.generate(None, sample)
            torch.cuda.synchronize()
    print("steps", g.beam_device_steps, "LM GEMM weight bytes", lm_gemm_bytes(lm))


def lm_gemm_bytes(lm):
    """bf16 bytes of every weight matrix an LM step streams (the layers' projections and the output projection; a tied projection
    streams the embedding table)."""
    return 2 * sum(p.numel() for n, p in lm.named_parameters() if p.dim() == 2 and "embed_tokens" not in n)


def split(path, nbytes):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    at = lambda key: [i for i, r in enumerate(rows) if key in r["Kernel_Name"]]     # noqa: E731
    embed, fuse, reorder = at("beam_embed_step_kernel"), at("beam_lm_logprobs_kernel"), at("beam_reorder_dev_kernel")
    assert len(embed) == 2 * len(fuse) == 2 * len(reorder), (len(embed), len(fuse), len(reorder))
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])              # noqa: E731
    out = []
    for s in range(len(fuse) // 2, len(fuse)):          # the second call
        a, b, c, e = embed[2 * s], embed[2 * s + 1], fuse[s], reorder[s]
        lm = rows[b:c]
        gemm = [dur(r) for r in lm if "skinny_gemm_kernel" in r["Kernel_Name"]]
        comb = sum(dur(r) for r in lm if "skinny_combine_kernel" in r["Kernel_Name"])
        out.append((sum(gemm), comb, sum(dur(r) for r in lm) - sum(gemm) - comb, sum(dur(r) for r in rows[a:b]),
                    sum(dur(r) for r in rows[c:e + 1]), int(rows[e]["End_Timestamp"]) - int(rows[a]["Start_Timestamp"]), len(gemm), len(lm)))
    med = lambda k: statistics.median(o[k] for o in out)                             # noqa: E731
    print(f"steps {len(out)}; per step, medians in us: LM skinny_gemm {med(0) / 1e3:.1f} ({int(med(6))} launches), LM skinny_combine "
          f"{med(1) / 1e3:.1f}, LM other (embed, LayerNorm, attention) {med(2) / 1e3:.1f} ({int(med(7))} LM launches in all), decoder "
          f"{med(3) / 1e3:.1f}, fuse + beam step + reorder {med(4) / 1e3:.1f}, first launch to last end {med(5) / 1e3:.1f}")
    print(f"LM GEMM weight bytes {nbytes}: {nbytes / med(0):.0f} GB/s over the GEMM kernels alone, {nbytes / (med(0) + med(1)):.0f} GB/s with "
          f"their combine kernels (MI355X HBM peak: 8000 GB/s)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--split", default=None, help="a kernel trace csv of the decode")
    ap.add_argument("--bytes", type=int, default=891502080, help="LM GEMM weight bytes (the decode prints them)")
    a = ap.parse_args()
    split(a.split, a.bytes) if a.split else decode()
