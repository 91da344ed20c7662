"""Timing of ASR beam search over a slot cache (SequenceGenerator(decode="slots")) against the concatenating cache it replaces
(decode="concat", the default).

Base size (t5_transformer_base, seeded random weights, eval), the 83-entry character dictionary of the ASR recipe, seeded clips of
10 s (S = 499 encoder frames), fp32 and bf16, bsz in {1, 8, 32}, beam in {1, 10}, CTC weight 0 and 0.5 (ctc_rows=True, so that every
sentence is scored against its own posterior; a configuration in which the random model leaves its CTC candidate list at every clip
seed -- beam 1 has 7 candidates -- is recorded as not measured).  max_len_b = min_len, so both arms take the same number of decoder steps whatever the
random model says.  Two arms, alternated in one process after a warm-up call of each: whole generate() calls, host clock around a call
that ends in a device synchronise.  Reported per configuration: the per-repeat times of both arms, the spread of the concat repeats,
the ratio of the medians, and whether every slots repeat beats every concat repeat.

    python tools/beam_slots_timing.py [--bsz 1 8 32] [--beam 1 10] [--dtype bf16 fp32] [--ctc 0 0.5] [--reps 5] [--steps 40] [--json out.json]

--kernel   st5_beam_cross_attn alone at the decode step's shapes (device events around groups of launches): time per launch and the
           once-per-sentence K|V bytes (n_sent x S x 2C elements) over it, against st5_decode_cross_attn on K|V replicated per
           hypothesis row (what the concatenating path's attention reads).
--count ARM  two calls of one arm in a fresh process, for a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/beam_slots_timing.py --count slots --bsz 8 --beam 10 --dtype bf16 --ctc 0"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import functional as Fn  # noqa: E402
from speech_rows_timing import RATE, batch, build  # noqa: E402

SECONDS = 10                 # (10 s * 16 kHz - 400) // 320 + 1 = 499 frames
ARMS = ["concat", "slots"]


def build_model(dev, dtype):
    from argparse import Namespace
    from speecht5_amd.task import SpeechT5Task
    return build(dev, dtype), SpeechT5Task.synthetic(Namespace()).target_dictionary


def generator(model, d, arm, beam, steps, ctc):
    from speecht5_amd.sequence_generator import SequenceGenerator
    kw = dict(beam_size=beam, max_len_a=0, max_len_b=steps, min_len=steps, decode=arm)
    if ctc > 0:
        kw.update(ctc_weight=ctc, ctc_rows=True)
    return SequenceGenerator([model], d, **kw)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def decodable_batch(model, gens, n, dev, arms=ARMS):
    """The first clip seed at which the arms decode every clip (a random model can pick a token outside its CTC candidate list, the
    generator's KeyError); doubles as the warm-up of those arms."""
    for seed in range(7, 27):
        wav, pad = batch(n, dev, seed=seed)
        sample = {"net_input": {"source": wav, "padding_mask": pad}}
        try:
            for arm in arms:
                gens[arm].generate(None, sample)
            return sample, seed
        except KeyError:
            continue
    raise RuntimeError("no clip seed in 7 .. 26 lets the arms decode every clip: a hypothesis left its CTC candidate list (KeyError)")


def kernel_times(dev, results):
    H, hd, S, C, beam = 12, 64, 499, 768, 10
    for dname, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        esz = 2 if dtype == torch.bfloat16 else 4
        for n_sent in (1, 8, 32):
            rows = n_sent * beam
            g = torch.Generator().manual_seed(n_sent)
            kv = torch.randn(n_sent * S, 6 * 2 * C, generator=g).to(dtype).to(dev)          # all six layers side by side
            q = torch.randn(rows, C, generator=g).to(dtype).to(dev)
            sent = torch.arange(n_sent, dtype=torch.int32, device=dev)
            kpm = torch.zeros(n_sent, S, dtype=torch.uint8, device=dev)
            rep = kv.view(n_sent, S, -1)[:, :, 2 * C:4 * C].repeat_interleave(beam, dim=0).reshape(rows * S, 2 * C).contiguous()
            kpm_rep = kpm.repeat_interleave(beam, dim=0).contiguous()
            ws_b = Fn.beam_cross_attn_ws(rows, S, H, hd, dev)
            ws_r = Fn.decode_cross_attn_ws(rows, S, H, hd, dev)
            fns = {"beam": lambda: Fn.beam_cross_attn(q, kv, 2 * C, sent, n_sent, beam, S, H, hd, kpm=kpm, ws=ws_b),
                   "rows": lambda: Fn.decode_cross_attn(q, rep, 0, S, H, hd, kpm=kpm_rep, ws=ws_r)}
            us = {k: [] for k in fns}
            for fn in fns.values():
                for _ in range(5):
                    fn()
            for _ in range(7):                                        # 7 groups of 20 launches per arm, the arms alternating
                for name, fn in fns.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        fn()
                    e1.record()
                    e1.synchronize()
                    us[name].append(e0.elapsed_time(e1) / 20 * 1e3)
            once = n_sent * S * 2 * C * esz
            b, r = statistics.median(us["beam"]), statistics.median(us["rows"])
            res = dict(mode="kernel", dtype=dname, n_sent=n_sent, beam=beam, S=S, H=H, beam_us=round(b, 2), rows_us=round(r, 2),
                       beam_us_all=[round(v, 2) for v in us["beam"]], rows_us_all=[round(v, 2) for v in us["rows"]],
                       kv_bytes_once_per_sentence=once, beam_GBps_of_once_bytes=round(once / (b * 1e-6) / 1e9, 1),
                       rows_GBps_of_replicated_bytes=round(once * beam / (r * 1e-6) / 1e9, 1), rows_over_beam=round(r / b, 2),
                       note="launch + combine launch per call, back to back on one stream; includes launch overhead")
            results.append(res)
            print(json.dumps(res), flush=True)
            del kv, rep
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsz", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--beam", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--dtype", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--ctc", type=float, nargs="+", default=[0.0, 0.5])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--count", default=None, choices=ARMS)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []

    def flush():
        if a.json and results:
            with open(a.json, "w") as f:
                json.dump(results, f, indent=1)

    if a.kernel:
        with torch.no_grad():
            kernel_times(dev, results)
        flush()
        return
    for dname in a.dtype:
        dtype = torch.float32 if dname == "fp32" else torch.bfloat16
        model, d = build_model(dev, dtype)
        assert len(d) == 83
        with torch.no_grad():
            for bsz in a.bsz:
                n = [SECONDS * RATE] * bsz
                for beam in a.beam:
                    for ctc in a.ctc:
                        gens = {arm: generator(model, d, arm, beam, a.steps, ctc) for arm in ARMS}
                        try:
                            sample, seed = decodable_batch(model, gens, n, dev, [a.count] if a.count else ARMS)
                        except RuntimeError as e:      # (beam 1 has 7 CTC candidates: the random model leaves them at every seed)
                            results.append(dict(dtype=dname, bsz=bsz, beam=beam, ctc_weight=ctc, not_measured=str(e)))
                            print(json.dumps(results[-1]), flush=True)
                            continue
                        fns = {arm: (lambda g=gens[arm]: g.generate(None, sample)) for arm in ARMS}
                        if a.count:
                            for _ in range(2):
                                timed(fns[a.count])
                            print(json.dumps(dict(mode="count", arm=a.count, bsz=bsz, beam=beam, dtype=dname, ctc_weight=ctc, calls=2,
                                                  steps=a.steps + 1, clip_seed=seed,
                                                  note="the arm's warm-up call (decodable_batch) is in the trace too: 3 calls")))
                            continue
                        times, outs = {arm: [] for arm in ARMS}, {}
                        for _ in range(a.reps):
                            for arm in ARMS:
                                t, outs[arm] = timed(fns[arm])
                                times[arm].append(t)
                        cc, sl = times["concat"], times["slots"]
                        same = [outs["concat"][b][0]["tokens"].tolist() == outs["slots"][b][0]["tokens"].tolist() for b in range(bsz)]
                        r = dict(dtype=dname, bsz=bsz, beam=beam, ctc_weight=ctc, S=499, steps=a.steps + 1, clip_seed=seed,
                                 concat_ms=[round(t * 1e3, 1) for t in cc], slots_ms=[round(t * 1e3, 1) for t in sl],
                                 concat_spread_ms=round((max(cc) - min(cc)) * 1e3, 1),
                                 concat_over_slots=round(statistics.median(cc) / statistics.median(sl), 3),
                                 every_slots_repeat_beats_every_concat_repeat=max(sl) < min(cc),
                                 slots_no_slower_than_concat_beyond_its_spread=statistics.median(sl) <= statistics.median(cc) + (max(cc) - min(cc)),
                                 same_best_hypothesis=f"{sum(same)} of {bsz}")
                        results.append(r)
                        print(json.dumps(r), flush=True)
                        flush()
                        del gens
                        torch.cuda.empty_cache()
        del model
        torch.cuda.empty_cache()
    Fn.set_compute_dtype(torch.float32)
    flush()


if __name__ == "__main__":
    main()
