"""What feeding a new batch to every replayed update costs (update.PretrainUpdate.set_source, csrc/batch_load.hip), at the shape
bench.py times: Base, bf16, 8 x 10 s of speech + 16 x 512 text tokens, side-by-side micro-batches, host prefetch on, one GPU.

update  three arms ALTERNATED in one process, each a PretrainUpdate of its own (bench.make_update: same seeds, same model), after
        three warm-up updates of each; one repeat = `--updates` replayed updates between two device synchronisations, host clock,
        reported as ms per update; every repeat is kept:
          no_source   the replay without a source (what bench.py times)
          feed        set_source over two alternating copies of the benched pair: one st5_batch_load is the graph's first node
          copy_       no source; in front of every replay one Tensor.copy_ per tensor leaf from the same alternating copies into
                      the update's tensors, enqueued on the graph's stream (the per-leaf form the load kernel replaces)
load    the st5_batch_load launch alone at the benched leaves: HIP events around single launches on an otherwise idle stream, and
        around groups of ten (per launch = group / 10), after a warm-up; also the per-leaf copy_ sequence the same way.

    python tools/batch_feed_timing.py [--reps 7] [--updates 20] [--json profiles/batch_feed_timing.json]"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from speecht5_amd import functional as Fn  # noqa: E402
from speecht5_amd.graph import BatchFeed  # noqa: E402


def clone(x):
    if torch.is_tensor(x):
        return x.clone()
    if isinstance(x, dict):
        return {k: clone(v) for k, v in x.items()}
    if isinstance(x, list):
        return [clone(v) for v in x]
    return x


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "all": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arms = {}
    for name in ("no_source", "feed", "copy_"):
        _, _, _, upd = bench.make_update(dev)
        copies = [[clone(s) for s in upd.micro] for _ in range(2)]
        if name == "feed":
            upd.set_source(itertools.cycle(copies))
        upd.prepare_graph()
        feed = upd.feed if name == "feed" else BatchFeed(upd.micro, dev)
        pairs = None
        if name == "copy_":
            pairs = [list(zip(feed.dst, BatchFeed(c, dev).dst)) for c in copies]
        arms[name] = (upd, feed, pairs, copies)
    leaves = [{"path": f"micro_batches[{i}]." + ".".join(map(str, k)), "bytes": n} for (i, k), n in zip(arms["feed"][1].paths, arms["feed"][1].nbytes)]
    turn = {"n": 0}

    def one_update(name):
        upd, feed, pairs, _ = arms[name]
        if pairs is not None:
            with torch.cuda.stream(upd.sg.stream):
                for d, s in pairs[turn["n"] & 1]:
                    d.copy_(s, non_blocking=True)
            turn["n"] += 1
        upd.update()

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
            arms[name][0].finish()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / a.updates)
    out = {"shape": "base bf16, 8 x 10 s speech + 16 x 512 text, side_by_side, prefetch_host", "gpu": torch.cuda.get_device_name(dev),
           "updates_per_repeat": a.updates, "leaves": leaves, "leaf_bytes": sum(l["bytes"] for l in leaves),
           "update_ms": {k: summary(v) for k, v in times.items()}}

    # ---- the load launch alone ----
    upd, feed, _, copies = arms["feed"]
    src = BatchFeed(copies[0], dev)
    col = torch.tensor([t.data_ptr() for t in src.dst], dtype=torch.int64).to(dev)
    _, dst, nbytes, prefix = feed.table()
    torch.cuda.synchronize()

    def launch():
        Fn.batch_load(col, dst, nbytes, prefix, feed.n_leaves, feed.total_chunks)

    def per_leaf():
        for d, s in zip(feed.dst, src.dst):
            d.copy_(s, non_blocking=True)

    def events(fn, n, group):
        res = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(group):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res.append(e0.elapsed_time(e1) * 1e3 / group)
        return res
    load = {}
    for what, fn in (("st5_batch_load", launch), ("copy_per_leaf", per_leaf)):
        events(fn, 5, 1)
        load[what] = {"single_us": summary(events(fn, max(a.reps, 7) * 3, 1)), "group_of_10_us_per_launch": summary(events(fn, max(a.reps, 7), 10))}
    out["load_us"] = load
    for upd, _, _, _ in arms.values():
        upd.close()
    txt = json.dumps(out, indent=1)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(txt + "\n")
    brief = {k: {m: round(v[m], 4) for m in ("median", "min", "max")} for k, v in out["update_ms"].items()}
    print(json.dumps({"update_ms": brief, "load_us": {k: round(v["single_us"]["median"], 2) for k, v in load.items()},
                      "leaves": len(leaves), "leaf_bytes": out["leaf_bytes"]}))


if __name__ == "__main__":
    main()
