"""Timing of batched waveform synthesis: the ragged post-net + HiFi-GAN (Postnet.forward_ragged, SpeechT5HifiGan.forward_ragged) against
the per-row loop, and T5TransformerModel.synthesize_batch end to end.

Base model (t5_transformer_base, seeded random weights, every dropout 0) for the post-net and the decode; full-size generator with
seeded weights; bf16 and fp32; B in {1, 8, 32}; seeded mel lengths in 100 ... 600 frames.  Arms, alternated in one process after a
warm-up call of each, host clock around calls that end in a device synchronise:
  * loop     per row Postnet.forward and vocoder.forward(mel_b): the way to B waveforms without this path, the baseline;
  * ragged   Postnet.forward_ragged + vocoder.forward_ragged;
  * padded   vocoder.forward on the zero-padded [B, L_max, 80] batch.  Its row ends are WRONG (padding leaks into them); it is
             here only as a yardstick of device work.
Once per dtype: synthesize_batch (decode + post-net + vocoder) in utterances/s beside decode-only generate_speech_batch, B = 32,
100-token texts, threshold 2.0 (100 decode steps = 200 mel frames per row).

    python tools/tts_wave_timing.py [--B 1 8 32] [--dtype bf16 fp32] [--reps 5] [--json out.json]

Kernel traces come from runs of their own (--count makes a warm-up call and two timed calls of one arm):
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/tts_wave_timing.py --count ragged --B 8 --dtype bf16"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import functional as Fn  # noqa: E402
from tools.tts_batch_timing import build, texts, timed  # noqa: E402


def vocoder_for(dev, seed=11):
    from speecht5_amd.hifigan import SpeechT5HifiGan
    torch.manual_seed(seed)
    m = SpeechT5HifiGan().eval()
    with torch.no_grad():
        for p in m.parameters():
            p.normal_(0.0, 0.03)
        m.conv_post.weight.normal_(0.0, 0.3)
        m.mean.normal_(0.0, 0.5)
        m.scale.uniform_(0.5, 1.5)
    return m.to(dev)


def mels_for(B, dev, seed=600):
    g = torch.Generator().manual_seed(seed + B)
    lengths = torch.randint(100, 601, (B,), generator=g).tolist()
    return [(torch.randn(n, 80, generator=g) * 0.8 - 0.5).to(dev) for n in lengths], lengths


def arm_fn(arm, post, voc, mels, lengths):
    if arm == "loop":
        return lambda: [voc(post(Fn.to_compute(m.unsqueeze(0))).squeeze(0)) for m in mels]
    if arm == "ragged":
        return lambda: voc.forward_ragged(post.forward_ragged(mels))
    padded = torch.zeros(len(mels), max(lengths), 80, device=mels[0].device)
    for b, m in enumerate(mels):
        padded[b, :lengths[b]] = m
    return lambda: voc(padded)


def summary(ts):
    return dict(median_ms=round(statistics.median(ts) * 1e3, 3), min_ms=round(min(ts) * 1e3, 3), max_ms=round(max(ts) * 1e3, 3),
                call_ms=[round(t * 1e3, 3) for t in ts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--dtype", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", default=None, choices=["loop", "ragged", "padded"])
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    arms = ["loop", "ragged", "padded"]
    results = []
    for dname in a.dtype:
        dtype = torch.float32 if dname == "fp32" else torch.bfloat16
        model = build(dev, dtype)
        post = model.speech_decoder_postnet.postnet
        voc = vocoder_for(dev)
        with torch.no_grad():
            if a.count:
                mels, lengths = mels_for(a.B[0], dev)
                fn = arm_fn(a.count, post, voc, mels, lengths)
                for _ in range(3):
                    timed(fn)
                print(json.dumps(dict(mode="count", arm=a.count, B=a.B[0], dtype=dname, calls=3, mel_frames=sum(lengths))))
                continue
            for B in a.B:
                mels, lengths = mels_for(B, dev)
                fns = {arm: arm_fn(arm, post, voc, mels, lengths) for arm in arms}
                for arm in arms:
                    timed(fns[arm])                          # warm-up
                times = {arm: [] for arm in arms}
                for _ in range(a.reps):
                    for arm in arms:
                        times[arm].append(timed(fns[arm])[0])
                for arm in arms:
                    r = dict(dtype=dname, B=B, arm=arm, mel_frames=sum(lengths), padded_frames=B * max(lengths), **summary(times[arm]))
                    r["ms_per_utt"] = round(r["median_ms"] / B, 3)
                    results.append(r)
                    print(json.dumps(r), flush=True)
                lo, rg = times["loop"], times["ragged"]
                cond = dict(dtype=dname, B=B, speedup_median=round(statistics.median(lo) / statistics.median(rg), 2),
                            every_ragged_faster_than_every_loop=max(rg) < min(lo), loop_spread_ms=round((max(lo) - min(lo)) * 1e3, 3),
                            ragged_minus_loop_median_ms=round((statistics.median(rg) - statistics.median(lo)) * 1e3, 3))
                results.append(cond)
                print(json.dumps(cond), flush=True)
            if not a.no_e2e:
                B = max(a.B)
                toks, spk = texts(B, dev)
                e2e = {"decode_only": lambda: model.generate_speech_batch(src_tokens=toks, spkembs=spk, threshold=2.0, need_attn=False),
                       "synthesize": lambda: model.synthesize_batch(src_tokens=toks, spkembs=spk, threshold=2.0, vocoder=voc)}
                for fn in e2e.values():
                    timed(fn)
                times = {k: [] for k in e2e}
                for _ in range(a.reps):
                    for k, fn in e2e.items():
                        times[k].append(timed(fn)[0])
                for k, ts in times.items():
                    r = dict(dtype=dname, B=B, arm=k, utt_per_s=round(B / statistics.median(ts), 2), **summary(ts))
                    results.append(r)
                    print(json.dumps(r), flush=True)
        del model, voc
        torch.cuda.empty_cache()
    Fn.set_compute_dtype(torch.float32)
    if a.json and results:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
