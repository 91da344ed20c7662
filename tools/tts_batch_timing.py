"""Timing of batched speech synthesis (T5TransformerModel.generate_speech_batch) against generate_speech looped over the rows.

Base size (t5_transformer_base, seeded random weights, every dropout 0), 100-token texts, threshold = 2.0 (the reference reads it for
both length ratios as well: exactly 100 decode steps per row), fp32 and bf16, B in {1, 8, 32}.  Three arms, alternated in one process
after a warm-up call of each:
  * loop       generate_speech on each of the B rows in turn;
  * batch      generate_speech_batch(need_attn=True);
  * batch_noattn  generate_speech_batch(need_attn=False).
Reported per (dtype, B, arm): utterances/s and ms per decode step (median and min / max over the repeats; host clock around a call
that ends in a device synchronise), host polls per call.

    python tools/tts_batch_timing.py [--B 1 8 32] [--dtype fp32 bf16] [--reps 5] [--json out.json]

Launches per decode step come from kernel traces of the --count mode, which makes two calls of one arm at threshold 2.0 (100
steps) or 1.0 (50 steps) in a fresh process; the difference in kernel dispatches between the two processes, over the 2 x 50 steps, is
what one step launches (set-up and encoder launches cancel):
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/tts_batch_timing.py --count batch --count-threshold 2.0 --B 8"""
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

T_TEXT, STEPS = 100, 100


def build(dev, dtype, seed=4246):
    from speecht5_amd.speecht5 import t5_transformer_base
    from speecht5_amd.task import SpeechT5Task
    Fn.set_compute_dtype(dtype)
    Fn.weight_cache.clear()
    args = Namespace(label_rates=50, sample_rate=16000, speech_odim=80, bert_init=True, use_codebook=False,
                     share_input_output_embed=True, encoder_layerdrop=0.0, decoder_layerdrop=0.0)
    t5_transformer_base(args)
    for k, v in list(vars(args).items()):
        if "dropout" in k and isinstance(v, float):
            setattr(args, k, 0.0)
    task = SpeechT5Task.synthetic(args)
    task.t5_task = "t2s"
    torch.manual_seed(seed)
    return task.build_model(args).to(dev).eval()


def texts(B, dev, seed=21):
    g = torch.Generator().manual_seed(seed)
    toks = torch.randint(4, 81, (B, T_TEXT), generator=g)
    toks[:, -1] = 2
    return toks.to(dev), torch.randn(B, 512, generator=g).to(dev)


def arm_fn(model, arm, toks, spk, threshold):
    if arm == "loop":
        return lambda: [model.generate_speech(src_tokens=toks[b:b + 1], spkembs=spk[b:b + 1], threshold=threshold)
                        for b in range(toks.shape[0])]
    return lambda: model.generate_speech_batch(src_tokens=toks, spkembs=spk, threshold=threshold, need_attn=arm == "batch")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--dtype", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", default=None, choices=["loop", "batch", "batch_noattn"])
    ap.add_argument("--count-threshold", type=float, default=2.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    arms = ["loop", "batch", "batch_noattn"]
    results = []
    for dname in a.dtype:
        dtype = torch.float32 if dname == "fp32" else torch.bfloat16
        model = build(dev, dtype)
        with torch.no_grad():
            if a.count:
                toks, spk = texts(a.B[0], dev)
                for _ in range(2):
                    timed(arm_fn(model, a.count, toks, spk, a.count_threshold))
                print(json.dumps(dict(mode="count", arm=a.count, B=a.B[0], dtype=dname, calls=2, threshold=a.count_threshold)))
                continue
            for B in a.B:
                toks, spk = texts(B, dev)
                fns = {arm: arm_fn(model, arm, toks, spk, 2.0) for arm in arms}
                for arm in arms:                              # warm-up
                    _, out = timed(fns[arm])
                    lens = [o[0].shape[0] // model.reduction_factor for o in out]
                    assert lens == [STEPS] * B, (arm, lens)
                times = {arm: [] for arm in arms}
                polls = {arm: None for arm in arms}
                for _ in range(a.reps):
                    for arm in arms:
                        dt, _ = timed(fns[arm])
                        times[arm].append(dt)
                        polls[arm] = getattr(model, "tts_polls", None) if arm != "loop" else STEPS * B
                    print(f"# {dname} B={B} repeat {len(times['loop'])}: " + ", ".join(f"{k} {v[-1]:.3f} s" for k, v in times.items()),
                          flush=True)
                for arm in arms:
                    ts = times[arm]
                    med = statistics.median(ts)
                    steps = STEPS * B if arm == "loop" else STEPS
                    r = dict(dtype=dname, B=B, arm=arm, utt_per_s=round(B / med, 3), utt_per_s_min=round(B / max(ts), 3),
                             utt_per_s_max=round(B / min(ts), 3), ms_per_step=round(med / steps * 1e3, 4),
                             call_s=[round(t, 4) for t in ts], host_polls_per_call=polls[arm], decode_steps_per_call=steps)
                    results.append(r)
                    print(json.dumps(r), flush=True)
                lp = next(r for r in results if r["dtype"] == dname and r["B"] == B and r["arm"] == "loop")
                for arm in arms[1:]:
                    br = next(r for r in results if r["dtype"] == dname and r["B"] == B and r["arm"] == arm)
                    br["speedup_vs_loop"] = round(br["utt_per_s"] / lp["utt_per_s"], 2)
                    print(json.dumps(dict(dtype=dname, B=B, arm=arm, speedup_vs_loop=br["speedup_vs_loop"])), flush=True)
        del model
        torch.cuda.empty_cache()
    Fn.set_compute_dtype(torch.float32)
    if a.json and results:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
