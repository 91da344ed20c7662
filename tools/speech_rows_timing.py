"""Timing of the length-exact batched speech encoding (T5TransformerModel.forward_encoder_rows) against the per-clip loop it replaces.

Base size (t5_transformer_base, seeded random weights, eval), fp32 and bf16, B in {1, 8, 32}, two seeded length sets:
  * uniform   clip lengths uniform in 2 ... 10 s;
  * sorted    adjacent lengths after sorting: the longest clip and B - 1 more within 10 % below it.
Three arms, alternated in one process after a warm-up call of each:
  * loop      what _encode_rows did before forward_encoder_rows: the lengths from the mask, then forward_encoder on each unpadded
              clip in turn with its slice of the mask;
  * rows      forward_encoder_rows on the right-padded batch;
  * padded    forward_encoder on the right-padded batch, for scale: the reference's batch, which is NOT exact per row.
Every timed call gets a FRESH padding-mask tensor (cloned outside the timed region), as a caller with a new batch has: whatever an arm
remembers on the mask tensor (the host copy, the row lengths) is paid inside every timed call.
Reported per (dtype, B, lengths, arm): ms per call (median, min, max over the repeats; host clock around a call that ends in a device
synchronise), clips/s, and the padded-work fraction B * n_max / sum(n_b) of the length set.

    python tools/speech_rows_timing.py [--B 1 8 32] [--dtype bf16 fp32] [--reps 5] [--json out.json]

Kernel launches per arm come from a trace of the --count mode (two calls of one arm in a fresh process):
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/speech_rows_timing.py --count rows --B 8 --dtype bf16"""
import argparse
import json
import os
import statistics
import sys
import time
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import functional as Fn  # noqa: E402

RATE = 16000


def build(dev, dtype, seed=4246):
    from speecht5_amd.speecht5 import t5_transformer_base
    from speecht5_amd.task import SpeechT5Task
    Fn.set_compute_dtype(dtype)
    Fn.weight_cache.clear()
    args = Namespace(label_rates=50, sample_rate=RATE, speech_odim=80, bert_init=True, use_codebook=False,
                     share_input_output_embed=True, encoder_layerdrop=0.0, decoder_layerdrop=0.0)
    t5_transformer_base(args)
    for k, v in list(vars(args).items()):
        if "dropout" in k and isinstance(v, float):
            setattr(args, k, 0.0)
    task = SpeechT5Task.synthetic(args)
    task.t5_task = "s2t"
    torch.manual_seed(seed)
    return task.build_model(args).to(dev).eval()


def lengths(kind, B, seed=31):
    g = torch.Generator().manual_seed(seed + B)
    if kind == "uniform":
        return [int(v) for v in torch.randint(2 * RATE, 10 * RATE + 1, (B,), generator=g)]
    top = 10 * RATE
    return [top] + sorted((int(v) for v in torch.randint(int(0.9 * top), top + 1, (B - 1,), generator=g)), reverse=True)


def batch(n, dev, seed=7):
    g = torch.Generator().manual_seed(seed)
    wav = torch.zeros(len(n), max(n))
    pad = torch.ones(len(n), max(n), dtype=torch.bool)
    for b, m in enumerate(n):
        wav[b, :m] = torch.randn(m, generator=g) * 0.1
        pad[b, :m] = False
    return wav.to(dev), pad.to(dev)


def loop_encode(model, source, padding_mask):
    """The speech branch of _encode_rows as it was before forward_encoder_rows."""
    B = source.size(0)
    n = (~padding_mask.bool()).sum(1).tolist()
    outs = []
    for b in range(B):
        outs.append(model.forward_encoder(source[b:b + 1, :n[b]], padding_mask=padding_mask[b:b + 1, :n[b]])["encoder_out"][0])
    return outs


def arm_fn(model, arm, wav):
    if arm == "loop":
        return lambda pad: loop_encode(model, wav, pad)
    if arm == "rows":
        return lambda pad: model.forward_encoder_rows(wav, padding_mask=pad)["encoder_out"][0]
    return lambda pad: model.forward_encoder(wav, padding_mask=pad)["encoder_out"][0]


def timed(fn, pad):
    fresh = pad.clone()                          # (a new mask tensor per call: nothing remembered on it from the call before)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(fresh)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--dtype", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--lengths", nargs="+", default=["uniform", "sorted"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", default=None, choices=["loop", "rows", "padded"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    arms = ["loop", "rows", "padded"]
    results = []
    for dname in a.dtype:
        dtype = torch.float32 if dname == "fp32" else torch.bfloat16
        model = build(dev, dtype)
        with torch.no_grad():
            if a.count:
                n = lengths(a.lengths[0], a.B[0])
                wav, pad = batch(n, dev)
                fn = arm_fn(model, a.count, wav)
                for _ in range(2):
                    timed(fn, pad)
                print(json.dumps(dict(mode="count", arm=a.count, B=a.B[0], dtype=dname, lengths=a.lengths[0], calls=2)))
                continue
            for B in a.B:
                for kind in a.lengths:
                    n = lengths(kind, B)
                    frac = round(B * max(n) / sum(n), 4)
                    wav, pad = batch(n, dev)
                    fns = {arm: arm_fn(model, arm, wav) for arm in arms}
                    for arm in arms:                              # warm-up
                        timed(fns[arm], pad)
                    times = {arm: [] for arm in arms}
                    for _ in range(a.reps):
                        for arm in arms:
                            times[arm].append(timed(fns[arm], pad)[0])
                    for arm in arms:
                        ts = times[arm]
                        med = statistics.median(ts)
                        r = dict(dtype=dname, B=B, lengths=kind, arm=arm, padded_work=frac, ms=round(med * 1e3, 3), ms_min=round(min(ts) * 1e3, 3),
                                 ms_max=round(max(ts) * 1e3, 3), clips_per_s=round(B / med, 2), call_ms=[round(t * 1e3, 3) for t in ts])
                        results.append(r)
                        print(json.dumps(r), flush=True)
                    lp, rw = times["loop"], times["rows"]
                    s = dict(dtype=dname, B=B, lengths=kind, speedup_rows_vs_loop=round(statistics.median(lp) / statistics.median(rw), 2),
                             every_rows_repeat_beats_every_loop_repeat=max(rw) < min(lp))
                    results.append(s)
                    print(json.dumps(s), flush=True)
        del model
        torch.cuda.empty_cache()
    Fn.set_compute_dtype(torch.float32)
    if a.json and results:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
