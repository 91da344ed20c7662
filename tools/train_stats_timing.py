"""What the training statistics of the replayed update cost (update.PretrainUpdate(stats=True), csrc/train_stats.hip), at the shape
bench.py times: Base, bf16, 8 x 10 s of speech + 16 x 512 text tokens, side-by-side micro-batches, host prefetch on, one GPU.

update  three arms ALTERNATED in one process, each a PretrainUpdate of its own (bench.make_update: same seeds, same model), after
        three warm-up updates of each; one repeat = `--updates` replayed updates between two device synchronisations, host clock,
        reported as ms per update; every repeat is kept:
          stats_off   the replay as bench.py times it
          stats_on    stats=True: one st5_stats_record as the graph's last node, one copy of the ring every stats_rows // 2 updates,
                      logging_outputs() after every update
          copy_       stats off; behind every replay one Tensor.copy_ per cell from a device scalar of the cell's type into a row of
                      a device ring, on the graph's stream (the per-scalar form the record kernel replaces; the scalars are stand-ins
                      of the logged ones' types: those live inside the graph's pool, out of Python's reach)
record  the st5_stats_record launch alone at the update's cell layout: HIP events around single launches on an otherwise idle stream,
        and around groups of ten (per launch = group / 10), after a warm-up; also the per-cell copy_ sequence the same way.

    python tools/train_stats_timing.py [--reps 7] [--updates 20] [--json profiles/train_stats_timing.json]"""
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
from speecht5_amd import functional as Fn  # noqa: E402
from speecht5_amd import update as U  # noqa: E402
from speecht5_amd.train_stats import TYPE_CODES  # noqa: E402


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "all": v}


def make(dev, stats):
    """bench.make_update's update, built with stats=True where asked (make_update has no such argument: bench.py does not change)."""
    orig = U.PretrainUpdate
    if stats:
        U.PretrainUpdate = functools.partial(orig, stats=True)
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
    for name in ("stats_off", "stats_on", "copy_"):
        upd = make(dev, name == "stats_on")
        upd.prepare_graph()
        arms[name] = upd
    rec = arms["stats_on"].stats
    types, paths, rows = list(rec.cell_types), list(rec.paths), rec.rows
    n = len(types)
    # the per-cell form: one stand-in scalar per cell, one copy_ (a conversion kernel) per cell into the row of a ring
    stand_ins = [torch.ones(1, dtype=t, device=dev) for t in types]
    ring_c = torch.zeros(rows, 1 + n, dtype=torch.float64, device=dev)
    turn = {"n": 0}
    harvested = {"n": 0}

    def per_cell():
        row = ring_c[turn["n"] % rows]
        for i, s in enumerate(stand_ins):
            row[1 + i:2 + i].copy_(s, non_blocking=True)
        turn["n"] += 1

    def one_update(name):
        upd = arms[name]
        upd.update()
        if name == "copy_":
            with torch.cuda.stream(upd.sg.stream):
                per_cell()
        elif name == "stats_on":
            harvested["n"] += len(upd.logging_outputs())

    for name in arms:
        for _ in range(3):
            one_update(name)
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(a.reps):
        for name in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.updates):
                one_update(name)
            arms[name].finish()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / a.updates)
    harvested["n"] += len(arms["stats_on"].logging_outputs())
    out = {"shape": "base bf16, 8 x 10 s speech + 16 x 512 text, side_by_side, prefetch_host", "gpu": torch.cuda.get_device_name(dev),
           "updates_per_repeat": a.updates, "stats_rows": rows, "cells": [{"path": p, "dtype": str(t)} for p, t in zip(paths, types)],
           "updates_harvested": harvested["n"], "updates_enqueued": rec.sched.enqueued,
           "update_ms": {k: summary(v) for k, v in times.items()}}
    off, on = out["update_ms"]["stats_off"], out["update_ms"]["stats_on"]
    out["on_minus_off_ms"] = on["median"] - off["median"]
    out["on_minus_off_in_spreads_of_off"] = (on["median"] - off["median"]) / off["spread"] if off["spread"] > 0 else None

    # ---- the record launch alone ----
    col = torch.tensor([s.data_ptr() for s in stand_ins], dtype=torch.int64).to(dev)
    codes = torch.tensor([TYPE_CODES[t] for t in types], dtype=torch.int32).to(dev)
    ring = torch.zeros(rows, 1 + n, dtype=torch.int64, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def launch():
        Fn.stats_record(col, codes, ring, counter, rows, n)

    def events(fn, reps, group):
        res = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(group):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res.append(e0.elapsed_time(e1) * 1e3 / group)
        return res
    record = {}
    for what, fn in (("st5_stats_record", launch), ("copy_per_cell", per_cell)):
        events(fn, 5, 1)
        record[what] = {"single_us": summary(events(fn, max(a.reps, 7) * 3, 1)), "group_of_10_us_per_launch": summary(events(fn, max(a.reps, 7), 10))}
    out["record_us"] = record
    for upd in arms.values():
        upd.close()
    txt = json.dumps(out, indent=1)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(txt + "\n")
    brief = {k: {m: round(v[m], 4) for m in ("median", "min", "max")} for k, v in out["update_ms"].items()}
    print(json.dumps({"update_ms": brief, "on_minus_off_in_spreads_of_off": out["on_minus_off_in_spreads_of_off"],
                      "record_us": {k: round(v["single_us"]["median"], 2) for k, v in record.items()}, "cells": n,
                      "harvested": harvested["n"], "enqueued": rec.sched.enqueued}))


if __name__ == "__main__":
    main()
