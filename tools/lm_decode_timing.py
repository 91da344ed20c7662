"""Device-event timing of the shallow-fusion LM (speecht5_amd/transformer_lm.py) at the transformer_lm_t5 size (20 layers, 1280 wide,
16 heads, FFN 6144; seeded random weights, V = 83 as the ASR character dictionary) in fp32 and bf16:

  * step_ms      one incremental decode_step at prefix length t (slot cache + ancestry table);
  * full_ms      the full-prefix recompute of the same HIP model on [rows, t] tokens -- the reference's call pattern
                 (SpeechT5/speecht5/sequence_generator.py:420-425);
  * attn_us      st5_lm_decode_attn alone (one layer), with the bytes it must read (rows x t position rows of 2C elements) over
                 its time against the 6.3 TB/s a copy reaches on the MI355X;
  * gemm_ms      the decode step's GEMMs (20 x (Q, KV, out, fc1, fc2) + output projection), per-launch device events, against the
                 weight-streaming floor (all weights read once per step at 6.3 TB/s).

    python tools/lm_decode_timing.py [--rows 5 40] [--t 32 300 620] [--dtype fp32 bf16] [--json out.json]

Every number is a median over repeats after warm-up."""
import argparse
import json
import os
import statistics
import sys
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import functional as Fn  # noqa: E402
from speecht5_amd import hip  # noqa: E402
from speecht5_amd.transformer_lm import TransformerLanguageModel  # noqa: E402

HBM = 6.3e12
REAL = dict(decoder_embed_dim=1280, decoder_attention_heads=16, decoder_layers=20, decoder_ffn_embed_dim=6144, activation_fn="gelu")
MAXLEN = 622     # --max-len-b 620 + 2


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[5, 40])
    ap.add_argument("--t", type=int, nargs="+", default=[32, 300, 620])
    ap.add_argument("--dtype", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lm = TransformerLanguageModel(Namespace(**REAL), vocab=83, pad=1).to(dev).eval()
    H, hd, C = 16, 80, 1280
    wbytes = sum(p.numel() for n, p in lm.named_parameters() if n.endswith("weight") and p.dim() == 2 and "embed_tokens" not in n)
    results = []
    for dname in a.dtype:
        dtype = torch.float32 if dname == "fp32" else torch.bfloat16
        esz = 4 if dtype == torch.float32 else 2
        Fn.set_compute_dtype(dtype)
        for rows in a.rows:
            state = lm.init_decode(rows, MAXLEN)
            for kv in state.kv:
                kv.normal_()
            tok = torch.randint(4, 83, (rows,), device=dev)
            for t in a.t:
                def step():
                    state.t = t - 1
                    lm.decode_step(tok, state)
                with torch.no_grad():
                    step_ms = timed(step, 3, a.reps)
                    toks = torch.randint(4, 83, (rows, t), device=dev)
                    toks[:, 0] = 2
                    full_ms = timed(lambda: lm(toks), 2, max(3, a.reps // 2))
                    q = torch.randn(rows, C, device=dev).to(dtype)
                    attn_ms = timed(lambda: Fn.lm_decode_attn(q, state.kv[0], state.anc, t, H, hd, state.ws), 5, 50)
                    hip.profiler.reset()
                    hip.profiler.enabled = True
                    step()
                    torch.cuda.synchronize()
                    hip.profiler.enabled = False
                    gemm_ms = sum(e0.elapsed_time(e1) for _, _, e0, e1, _ in hip.profiler.records)
                    n_gemm = len(hip.profiler.records)
                    hip.profiler.reset()
                abytes = rows * t * 2 * C * esz
                r = dict(dtype=dname, rows=rows, t=t, step_ms=round(step_ms, 4), full_ms=round(full_ms, 3),
                         full_over_step=round(full_ms / step_ms, 1), attn_us=round(attn_ms * 1e3, 2),
                         attn_TBps=round(abytes / (attn_ms * 1e-3) / 1e12, 2), attn_frac_of_6p3=round(abytes / (attn_ms * 1e-3) / HBM, 3),
                         gemm_ms=round(gemm_ms, 4), gemm_launches=n_gemm, weight_floor_ms=round(wbytes * esz / HBM * 1e3, 4),
                         gemm_over_floor=round(gemm_ms / (wbytes * esz / HBM * 1e3), 2))
                results.append(r)
                print(json.dumps(r), flush=True)
            del state
            torch.cuda.empty_cache()
    Fn.set_compute_dtype(torch.float32)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
