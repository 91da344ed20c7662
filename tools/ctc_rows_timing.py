"""Timing of batched joint CTC / attention beam search (SequenceGenerator(exact_rows=True, ctc_rows=True)) against the per-sentence
loop it replaces, and of the rows prefix-score kernel against the single-posterior one.

Base size (t5_transformer_base, seeded random weights, eval), the 83-entry character dictionary of the ASR recipe, seeded clips of
5 ... 15 s, beam 10, CTC weight 0.5 (70 CTC candidates per hypothesis), fp32 and bf16, B in {1, 8, 32}.  max_len_b = min_len, so both
arms take the same number of decoder steps whatever the random model says.  Two arms, alternated in one process after a warm-up
call of each:
  * loop     the default generator called once per sentence on the unpadded clip (what the recipe does with --batch-size 1);
  * rows     one call on the right-padded batch with exact_rows=True, ctc_rows=True.
Reported per (dtype, B, arm): ms per utterance (median, min, max over the repeats; host clock around a call that ends in a device
synchronise), and per (dtype, B) how many sentences get the same best hypothesis from both arms and the largest score distance.
A random model can pick a token outside its CTC candidate list (the generator's KeyError); the clip seed is advanced until the
per-sentence loop decodes every clip.

    python tools/ctc_rows_timing.py [--B 1 8 32] [--dtype bf16 fp32] [--reps 3] [--steps 30] [--json out.json]

--kernel   per-launch time (HIP events around 50 launches) of ctc_prefix_score_rows_kernel against ctc_prefix_score_kernel at the
           same nh, nc, T (every row on one sentence of T frames), at out_len 1.
--parity   the bit-for-bit comparison of tests/test_ctc_rows_gpu.py (rows entries against the single-posterior entries per
           sentence, and the float32 numpy reference) at the timed size: 32 ragged sentences, 320 rows, 70 candidates.
--count ARM  two calls of one arm in a fresh process, for a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/ctc_rows_timing.py --count rows --B 8 --dtype bf16"""
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

BEAM, CTC_WEIGHT = 10, 0.5


def lengths(B, seed=53):
    g = torch.Generator().manual_seed(seed + B)
    return [int(v) for v in torch.randint(5 * RATE, 15 * RATE + 1, (B,), generator=g)]


def build_model(dev, dtype):
    """The model of tools/speech_rows_timing.py and the target dictionary its task gave it (synthetic, 83 entries)."""
    from argparse import Namespace
    from speecht5_amd.task import SpeechT5Task
    return build(dev, dtype), SpeechT5Task.synthetic(Namespace()).target_dictionary


def generators(model, d, steps):
    from speecht5_amd.sequence_generator import SequenceGenerator
    kw = dict(beam_size=BEAM, max_len_a=0, max_len_b=steps, min_len=steps, ctc_weight=CTC_WEIGHT)
    return SequenceGenerator([model], d, **kw), SequenceGenerator([model], d, exact_rows=True, ctc_rows=True, **kw)


def arm_fn(model, gens, arm, wav, pad, n):
    loop_gen, rows_gen = gens
    if arm == "loop":
        def loop():
            out = []
            for b, m in enumerate(n):
                ni = {"source": wav[b:b + 1, :m], "padding_mask": pad[b:b + 1, :m]}
                out.append(loop_gen.generate([model], {"net_input": ni})[0])
            return out
        return loop
    return lambda: rows_gen.generate([model], {"net_input": {"source": wav, "padding_mask": pad}})


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def decodable_batch(model, gens, n, dev):
    """The first clip seed at which the per-sentence loop decodes every clip (doubles as that arm's warm-up)."""
    for seed in range(7, 27):
        wav, pad = batch(n, dev, seed=seed)
        try:
            arm_fn(model, gens, "loop", wav, pad, n)()
            return wav, pad, seed
        except KeyError:
            continue
    raise RuntimeError("no clip seed in 7 .. 26 lets the default generator decode every clip")


def kernel_times(dev):
    from speecht5_amd.sequence_generator import CTCPrefixScorer, CTCPrefixScorerRows
    V, nc, blank, eos = 83, 70, 82, 2
    res = []
    for T in (250, 750):
        g = torch.Generator().manual_seed(T)
        x = torch.log_softmax(torch.randn(T, V, generator=g) * 2.0, -1).to(dev)
        one = CTCPrefixScorer(x, blank, eos)
        rows = CTCPrefixScorerRows(x[None], torch.tensor([T], dtype=torch.int32), blank, eos)
        for nh in (10, 80, 320):
            cs = torch.stack([torch.randperm(V - 1, generator=g)[:nc] for _ in range(nh)]).to(dev)
            last = torch.randint(4, V - 1, (nh,), generator=g).to(dev)
            r_prev = one.initial_state()[None].repeat(nh, 1, 1)
            r_prev[:, :, 0] = r_prev[:, :, 1] - 1.0
            sent = torch.zeros(nh, dtype=torch.int32, device=dev)
            a = one.score(last, 1, cs, r_prev)
            b = rows.score(sent, last, 1, cs, r_prev)
            same = bool(torch.equal(a[0], b[0])) and bool(torch.equal(a[1], b[1].permute(0, 2, 1, 3)))
            del a, b
            fns = {"single": lambda: one.score(last, 1, cs, r_prev), "rows": lambda: rows.score(sent, last, 1, cs, r_prev)}
            ms = {name: [] for name in fns}
            for fn in fns.values():
                for _ in range(3):
                    fn()
            for _ in range(5):                                     # 5 groups of 10 launches per arm, the arms alternating
                for name, fn in fns.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(10):
                        fn()
                    e1.record()
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / 10)
            r = dict(mode="kernel", T=T, nh=nh, nc=nc, bit_equal=same, single_us=round(statistics.median(ms["single"]) * 1e3, 1),
                     rows_us=round(statistics.median(ms["rows"]) * 1e3, 1), single_us_all=[round(t * 1e3, 1) for t in ms["single"]],
                     rows_us_all=[round(t * 1e3, 1) for t in ms["rows"]])
            r["single_over_rows"] = round(r["single_us"] / r["rows_us"], 2)
            res.append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    return res


def parity(dev):
    from tests.test_ctc_rows_gpu import _chain
    n = [(m - 400) // 320 + 1 for m in lengths(32)]                # frames of the timed clips
    n[3] = 1
    sent = [s for s in range(32) for _ in range(BEAM)]
    g = torch.Generator().manual_seed(5)
    sent = [sent[i] for i in torch.randperm(len(sent), generator=g).tolist()]
    _chain(dev, n, 83, 70, sent, seed=91, steps=3)
    print(f"timed size: {len(n)} sentences of {min(n)} ... {max(n)} frames, {len(sent)} rows in shuffled order, 70 candidates, steps 0 - 2: "
          "initial states, log psi and the valid part of every state BIT-EQUAL to st5_ctc_initial_state / st5_ctc_prefix_score per "
          "sentence on x[s, :T_s]; float32 numpy rows reference within rtol 2e-5 / atol 2e-4; select equal to the gathered states")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--dtype", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--count", default=None, choices=["loop", "rows"])
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []
    if a.kernel:
        results += kernel_times(dev)
    if a.parity:
        parity(dev)
    if a.kernel or a.parity:
        a.dtype = []
    arms = ["loop", "rows"]
    for dname in a.dtype:
        dtype = torch.float32 if dname == "fp32" else torch.bfloat16
        model, d = build_model(dev, dtype)
        assert len(d) == 83
        gens = generators(model, d, a.steps)
        with torch.no_grad():
            for B in a.B:
                n = lengths(B)
                wav, pad, seed = decodable_batch(model, gens, n, dev)
                fns = {arm: arm_fn(model, gens, arm, wav, pad, n) for arm in arms}
                if a.count:
                    for _ in range(2):
                        timed(fns[a.count])
                    print(json.dumps(dict(mode="count", arm=a.count, B=B, dtype=dname, calls=2, steps=a.steps + 1, clip_seed=seed,
                                          note="the loop arm's warm-up pass over the clips is in the trace too")))
                    continue
                timed(fns["rows"])                                 # warm-up (the loop arm's was decodable_batch)
                times, outs = {arm: [] for arm in arms}, {}
                for _ in range(a.reps):
                    for arm in arms:
                        t, outs[arm] = timed(fns[arm])
                        times[arm].append(t)
                for arm in arms:
                    ts = [t / B for t in times[arm]]
                    r = dict(dtype=dname, B=B, arm=arm, steps=a.steps + 1, clip_seed=seed, seconds_of_audio=round(sum(n) / RATE, 1),
                             ms_per_utt=round(statistics.median(ts) * 1e3, 2), ms_per_utt_min=round(min(ts) * 1e3, 2),
                             ms_per_utt_max=round(max(ts) * 1e3, 2), call_ms=[round(t * 1e3, 1) for t in times[arm]])
                    results.append(r)
                    print(json.dumps(r), flush=True)
                lp, rw = times["loop"], times["rows"]
                same = [outs["loop"][b][0]["tokens"].tolist() == outs["rows"][b][0]["tokens"].tolist() for b in range(B)]
                dist = max(abs(float(outs["loop"][b][0]["score"]) - float(outs["rows"][b][0]["score"])) for b in range(B))
                s = dict(dtype=dname, B=B, speedup_rows_vs_loop=round(statistics.median(lp) / statistics.median(rw), 2),
                         every_rows_repeat_beats_every_loop_repeat=max(rw) < min(lp),
                         loop_spread_ms_per_utt=round((max(lp) - min(lp)) / B * 1e3, 2),
                         same_best_hypothesis=f"{sum(same)} of {B}", largest_best_score_distance=round(dist, 6))
                results.append(s)
                print(json.dumps(s), flush=True)
        del model, gens
        torch.cuda.empty_cache()
    Fn.set_compute_dtype(torch.float32)
    if a.json and results:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
