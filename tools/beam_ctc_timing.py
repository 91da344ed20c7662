"""Timing of joint CTC / attention beam search (ctc_weight 0.5, ctc_rows=True) with the step on the device
(SequenceGenerator(decode="device")) and replayed from a HIP graph (decode="graph") against decode="slots" with the same options (the
yardstick: the path these modes did not cover before).

Base size (t5_transformer_base, seeded random weights, eval), the 83-entry character dictionary of the ASR recipe, seeded clips of
10 s (S = 499 encoder frames), bf16 by default, (sentences x beam) in 1 x 1, 1 x 5, 1 x 10, 8 x 1, 8 x 10.  max_len_b = min_len, so
all arms take the same number of decoder steps whatever the random model says.  A random model's next-token distribution is nearly
flat, and under a flat distribution a hypothesis soon leaves its 7 x beam CTC candidates, which the generator answers with KeyError
by design; --temperature (the same for every arm) sharpens it so that the candidates stay ahead: the values are tried in order
(default 0.25, then 0.05: beam 1 has 7 candidates only) and the first under which no arm raises is measured and recorded, with the
ones that raised; a shape under which every temperature raises is reported on stderr and the tool exits non-zero.  Three arms, alternated in one process after a warm-up call of each: whole generate() calls, host clock around a
call that ends in a device synchronise.  Reported per shape: the per-repeat times of every arm, the spread of the slots repeats, the
ratios of the medians, how many best hypotheses agree with slots.

    python tools/beam_ctc_timing.py [--shapes 1x1 1x5 1x10 8x1 8x10] [--dtype bf16] [--reps 5] [--steps 40] [--json out.json]"""
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
CTC_WEIGHT = 0.5


def measure(gens, sample, reps):
    """(outs, times) of `reps` alternated whole generate() calls per arm after a warm-up call of each."""
    fns = {arm: (lambda g=gens[arm]: g.generate(None, sample)) for arm in ARMS}
    outs = {arm: timed(fns[arm])[1] for arm in ARMS}
    times = {arm: [] for arm in ARMS}
    for _ in range(reps):
        for arm in ARMS:
            t, outs[arm] = timed(fns[arm])
            times[arm].append(t)
    return outs, times


def generator(model, d, arm, beam, steps, temperature):
    from speecht5_amd.sequence_generator import SequenceGenerator
    return SequenceGenerator([model], d, beam_size=beam, max_len_a=0, max_len_b=steps, min_len=steps, decode=arm, ctc_weight=CTC_WEIGHT,
                             ctc_rows=True, temperature=temperature)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1x1", "1x5", "1x10", "8x1", "8x10"], help="sentences x beam")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--temperature", type=float, nargs="+", default=[0.25, 0.05])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    results, failed = [], []
    dtype = torch.float32 if a.dtype == "fp32" else torch.bfloat16
    model, d = build_model(dev, dtype)
    assert len(d) == 83
    med = statistics.median
    with torch.no_grad():
        for shape in a.shapes:
            bsz, beam = (int(v) for v in shape.split("x"))
            wav, pad = batch([SECONDS * RATE] * bsz, dev, seed=7)
            sample = {"net_input": {"source": wav, "padding_mask": pad}}
            ens = generator(model, d, "slots", beam, a.steps, 1.0).model         # (the generator's ensemble wrapper: its encoder call)
            frames = int(model.get_normalized_probs_for_ctc(ens.forward_encoder(sample["net_input"])[0], log_probs=True).shape[0])
            del ens
            r = dict(dtype=a.dtype, bsz=bsz, beam=beam, S=frames, steps=a.steps + 1, ctc_weight=CTC_WEIGHT, ctc_rows=True,
                     temperature=None, key_error_at_temperature=[])
            for temperature in a.temperature:
                gens = {arm: generator(model, d, arm, beam, a.steps, temperature) for arm in ARMS}
                try:
                    outs, times = measure(gens, sample, a.reps)
                except KeyError:
                    torch.cuda.synchronize()
                    r["key_error_at_temperature"].append(temperature)
                    continue
                sl, de, gr = times["slots"], times["device"], times["graph"]
                same = {arm: sum(outs["slots"][b][0]["tokens"].tolist() == outs[arm][b][0]["tokens"].tolist() for b in range(bsz))
                        for arm in ("device", "graph")}
                g = gens["graph"]
                r.update(temperature=temperature, slots_ms=[round(t * 1e3, 1) for t in sl], device_ms=[round(t * 1e3, 1) for t in de],
                         graph_ms=[round(t * 1e3, 1) for t in gr], slots_spread_ms=round((max(sl) - min(sl)) * 1e3, 1),
                         slots_over_device=round(med(sl) / med(de), 3), slots_over_graph=round(med(sl) / med(gr), 3),
                         every_graph_repeat_beats_every_slots_repeat=max(gr) < min(sl),
                         graph_polls=g.beam_polls, graph_replays=g.beam_graph_replays,
                         same_best_hypothesis_as_slots={k: f"{v} of {bsz}" for k, v in same.items()})
                break
            results.append(r)
            print(json.dumps(r), flush=True)
            if r["temperature"] is None:
                failed.append(shape)
                print(f"beam_ctc_timing: {shape} NOT MEASURED: every arm set raised the CTC KeyError at temperatures {a.temperature}",
                      file=sys.stderr, flush=True)
            if a.json:
                with open(a.json, "w") as f:
                    json.dump(results, f, indent=1)
            del gens
            torch.cuda.empty_cache()
    Fn.set_compute_dtype(torch.float32)
    if failed:
        sys.exit(f"beam_ctc_timing: no timing for {failed}; pass a sharper --temperature")


if __name__ == "__main__":
    main()
