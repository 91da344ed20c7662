"""What the finite-gradient guard of the Adam step costs (update.PretrainUpdate(nonfinite="skip"), st5_adam_step_guard), at the shape
bench.py times: Base, bf16, 8 x 10 s of speech + 16 x 512 text tokens, side-by-side micro-batches, host prefetch on, one GPU.

Two arms ALTERNATED in one process, each a PretrainUpdate of its own (bench.make_update: same seeds, same model), after three warm-up
updates of each; one repeat = `--updates` replayed updates between two device synchronisations, host clock, reported as ms per update;
every repeat is kept:
    guard_off   the replay as bench.py times it (st5_adam_step_pair)
    guard_on    nonfinite="skip": the same graph with st5_adam_step_guard as its Adam node (the norm is computed in both: bench clips)
The bar: the two medians differ by less than the larger min-max spread of the two arms.

    python tools/nonfinite_guard_timing.py [--reps 7] [--updates 20] [--json profiles/nonfinite_guard_timing.json]"""
import argparse
import functools
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from speecht5_amd import update as U  # noqa: E402


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "all": v}


def make(dev, guard):
    """bench.make_update's update, built with nonfinite="skip" where asked (make_update has no such argument: bench.py does not change)."""
    orig = U.PretrainUpdate
    if guard:
        U.PretrainUpdate = functools.partial(orig, nonfinite="skip")
    try:
        return bench.make_update(dev)[3]
    finally:
        U.PretrainUpdate = orig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arms = {}
    for name in ("guard_off", "guard_on"):
        upd = make(dev, name == "guard_on")
        upd.prepare_graph()
        arms[name] = upd
    assert arms["guard_on"].opt.guard is not None and arms["guard_off"].opt.guard is None
    for upd in arms.values():
        for _ in range(3):
            upd.update()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(a.reps):
        for name, upd in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.updates):
                upd.update()
            upd.finish()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / a.updates)
    out = {"shape": "base bf16, 8 x 10 s speech + 16 x 512 text, side_by_side, prefetch_host", "gpu": torch.cuda.get_device_name(dev),
           "updates_per_repeat": a.updates, "repeats": a.reps, "order": "guard_off, guard_on alternated, every repeat kept",
           "parameters": int(arms["guard_on"].opt.pflat.numel()),
           "update_ms": {k: summary(v) for k, v in times.items()},
           "skipped_by_guard_on": arms["guard_on"].opt.skipped()}
    off, on = out["update_ms"]["guard_off"], out["update_ms"]["guard_on"]
    out["on_minus_off_ms"] = on["median"] - off["median"]
    out["larger_spread_ms"] = max(on["spread"], off["spread"])
    out["within_the_bar"] = abs(out["on_minus_off_ms"]) < out["larger_spread_ms"]
    for upd in arms.values():
        upd.close()
    txt = json.dumps(out, indent=1)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(txt + "\n")
    print(json.dumps({"update_ms": {k: {m: round(v[m], 4) for m in ("median", "min", "max", "spread")} for k, v in out["update_ms"].items()},
                      "on_minus_off_ms": round(out["on_minus_off_ms"], 4), "within_the_bar": out["within_the_bar"],
                      "skipped": out["skipped_by_guard_on"]}))


if __name__ == "__main__":
    main()
