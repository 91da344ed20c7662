"""Timing of ASR beam search with the beam step on the device (SequenceGenerator(decode="device")) and replayed from a HIP graph
(decode="graph") against the slot-cache loop it grows out of (decode="slots", the yardstick).

Base size (t5_transformer_base, seeded random weights, eval), the 83-entry character dictionary of the ASR recipe, seeded clips of
10 s (S = 499 encoder frames), bf16 by default, bsz in {1, 8, 32}, beam in {1, 10}.  max_len_b = min_len, so all arms take the same
number of decoder steps whatever the random model says.  Three arms, alternated in one process after a warm-up call of each: whole
generate() calls, host clock around a call that ends in a device synchronise.  Reported per configuration: the per-repeat times of
every arm, the spread of the slots repeats, the ratios of the medians, whether every graph repeat beats every slots repeat.

    python tools/beam_device_timing.py [--bsz 1 8 32] [--beam 1 10] [--dtype bf16] [--reps 5] [--steps 40] [--json out.json]

--count ARM  two calls of one arm in a fresh process, for a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/beam_device_timing.py --count graph --bsz 8 --beam 10"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import functional as Fn  # noqa: E402
from beam_slots_timing import SECONDS, build_model, timed  # noqa: E402
from speech_rows_timing import RATE, batch  # noqa: E402

ARMS = ["slots", "device", "graph"]


def generator(model, d, arm, beam, steps):
    from speecht5_amd.sequence_generator import SequenceGenerator
    return SequenceGenerator([model], d, beam_size=beam, max_len_a=0, max_len_b=steps, min_len=steps, decode=arm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsz", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--beam", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--dtype", nargs="+", default=["bf16"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--count", default=None, choices=ARMS)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []

    def flush():
        if a.json and results:
            with open(a.json, "w") as f:
                json.dump(results, f, indent=1)

    for dname in a.dtype:
        dtype = torch.float32 if dname == "fp32" else torch.bfloat16
        model, d = build_model(dev, dtype)
        assert len(d) == 83
        with torch.no_grad():
            for bsz in a.bsz:
                wav, pad = batch([SECONDS * RATE] * bsz, dev, seed=7)
                sample = {"net_input": {"source": wav, "padding_mask": pad}}
                for beam in a.beam:
                    arms = [a.count] if a.count else ARMS
                    gens = {arm: generator(model, d, arm, beam, a.steps) for arm in arms}
                    fns = {arm: (lambda g=gens[arm]: g.generate(None, sample)) for arm in arms}
                    outs = {arm: timed(fns[arm])[1] for arm in arms}          # the warm-up call of each arm
                    if a.count:
                        for _ in range(2):
                            timed(fns[a.count])
                        print(json.dumps(dict(mode="count", arm=a.count, bsz=bsz, beam=beam, dtype=dname, calls=3, steps=a.steps + 1,
                                              note="the arm's warm-up call is in the trace too: 3 calls")))
                        continue
                    times = {arm: [] for arm in ARMS}
                    for _ in range(a.reps):
                        for arm in ARMS:
                            t, outs[arm] = timed(fns[arm])
                            times[arm].append(t)
                    sl, de, gr = times["slots"], times["device"], times["graph"]
                    med = statistics.median
                    same = {arm: sum(outs["slots"][b][0]["tokens"].tolist() == outs[arm][b][0]["tokens"].tolist() for b in range(bsz))
                            for arm in ("device", "graph")}
                    g = gens["graph"]
                    r = dict(dtype=dname, bsz=bsz, beam=beam, S=499, steps=a.steps + 1,
                             slots_ms=[round(t * 1e3, 1) for t in sl], device_ms=[round(t * 1e3, 1) for t in de],
                             graph_ms=[round(t * 1e3, 1) for t in gr], slots_spread_ms=round((max(sl) - min(sl)) * 1e3, 1),
                             slots_over_device=round(med(sl) / med(de), 3), slots_over_graph=round(med(sl) / med(gr), 3),
                             every_graph_repeat_beats_every_slots_repeat=max(gr) < min(sl),
                             graph_no_slower_than_slots_beyond_its_spread=med(gr) <= med(sl) + (max(sl) - min(sl)),
                             graph_polls=g.beam_polls, graph_replays=g.beam_graph_replays,
                             same_best_hypothesis_as_slots={k: f"{v} of {bsz}" for k, v in same.items()})
                    results.append(r)
                    print(json.dumps(r), flush=True)
                    flush()
                    del gens, fns
                    torch.cuda.empty_cache()
        del model
        torch.cuda.empty_cache()
    Fn.set_compute_dtype(torch.float32)
    flush()


if __name__ == "__main__":
    main()
