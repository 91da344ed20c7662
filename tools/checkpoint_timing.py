"""What a checkpoint costs the running update (update.PretrainUpdate.snapshot / save_checkpoint): the benched pre-training
update (bench.make_update: Base, bf16, BASELINE.json cfg 2, side by side), replayed with prefetch_host=False -- the form a snapshot
needs -- on one GPU.

update    ONE update object, two kinds of repeat ALTERNATED after three warm-up replays: `--updates` replays, and the same with one
          snapshot() behind the middle one.  A repeat is timed on the host clock from its first update() to the end of the UPDATE's
          stream (not of the device: the copy to the host runs on a side stream and may outlive the repeat -- that is the claim under
          test); ms per update; every repeat is kept.  result() is taken outside the timed region.
launches  HIP events on the update's stream around the snapshot's two launches together (st5_batch_load into the shadow,
          st5_state_digest over it), with the bytes each moves; the per-kernel split comes from a separate
          `rocprofv3 --kernel-trace --stats -- python tools/checkpoint_timing.py --trace-only` run (three replays, one snapshot,
          three replays) whose kernel statistics `--stats-csv` merges into the JSON.
copy      HIP events on the side stream around the device-to-host copy of shadow and digest cells.
save      wall time of save_checkpoint(path) on local disk (snapshot, wait, host digests, torch.save, fsync, replace) and of
          load_checkpoint(path) (torch.load + digests), once each, after the repeats.

    python tools/checkpoint_timing.py [--reps 5] [--updates 20] [--json profiles/checkpoint_timing.json] [--dir /tmp]
           [--stats-csv kernel_stats.csv] [--bench-json bench_lines.json] [--commits parent,this]"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    return {"mean": statistics.mean(v), "median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "all": v}


def timed_snapshot(upd):
    """upd.snapshot() with HIP events around its two launches and around the copy (the same enqueue order as checkpoint.snapshot:
    the events are recorded on the streams it uses, before and behind it)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(upd.stream):
        e0.record()
    h = upd.snapshot()
    with torch.cuda.stream(upd.stream):
        e1.record()
    return h, e0, e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--dir", default=None, help="directory of the checkpoint file (default: a temporary directory)")
    ap.add_argument("--trace-only", action="store_true", help="three replays, one snapshot, three replays: the run to put under rocprofv3")
    ap.add_argument("--stats-csv", default=None, help="kernel statistics of the rocprofv3 run, merged into the JSON")
    ap.add_argument("--bench-json", default=None, help="a JSON file of bench.py result lines {'parent': [...], 'this': [...]}, merged in")
    ap.add_argument("--commits", default="")
    a = ap.parse_args()
    import bench
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _, _, _, upd = bench.make_update(dev, prefetch_host=False)
    upd.prepare_graph()
    for _ in range(3):
        upd.update()
    upd.finish()
    upd.stream.synchronize()
    if a.trace_only:
        h = upd.snapshot()
        for _ in range(3):
            upd.update()
        upd.finish()
        h.result()
        torch.cuda.synchronize()
        upd.close()
        print(json.dumps({"trace_only": True}))
        return
    sh_bytes = None
    times = {"plain": [], "with_snapshot": []}
    launches_ms, copy_ms, result_s = [], [], []
    for _ in range(a.reps):
        for kind in ("plain", "with_snapshot"):
            torch.cuda.synchronize()
            h = None
            t0 = time.perf_counter()
            for k in range(a.updates):
                upd.update()
                if kind == "with_snapshot" and k == a.updates // 2 - 1:
                    h, e0, e1 = timed_snapshot(upd)
            upd.finish()
            upd.stream.synchronize()
            times[kind].append((time.perf_counter() - t0) * 1e3 / a.updates)
            if h is not None:
                t1 = time.perf_counter()
                h.result()
                result_s.append(time.perf_counter() - t1)
                launches_ms.append(e0.elapsed_time(e1))
    # the copy alone, on the side stream, with nothing else running: the shadow still holds the last snapshot
    sh = upd._shadow
    sh_bytes = sum(sh.nbytes)
    for _ in range(3):
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(sh.side):
            c0.record()
            sh.host.copy_(sh.dev, non_blocking=True)
            sh.cells_host.copy_(sh.cells, non_blocking=True)
            c1.record()
        c1.synchronize()
        copy_ms.append(c0.elapsed_time(c1))
    wflat_bytes = upd.opt.wflat.numel() * 2 if upd.opt.mirror is not None else 0
    out = {"shape": "bench.make_update: t5_transformer_base bf16, BASELINE.json cfg 2, side_by_side, graph, prefetch_host=False",
           "gpu": torch.cuda.get_device_name(dev), "updates_per_repeat": a.updates, "commits": a.commits,
           "update_ms": {k: summary(v) for k, v in times.items()},
           "snapshot": {"shadow_bytes": sh_bytes, "batch_load_bytes_moved": 2 * sh_bytes, "digest_bytes_read": sh_bytes + wflat_bytes,
                        "two_launches_ms_by_events": summary(launches_ms), "device_to_host_copy_ms_alone": summary(copy_ms),
                        "device_to_host_copy_GBps": sh_bytes / (statistics.median(copy_ms) * 1e-3) / 1e9,
                        "result_wait_and_host_digest_s": summary(result_s),
                        "per_kernel": "not measured (no --stats-csv given)"}}
    d = a.dir or tempfile.mkdtemp()
    path = os.path.join(d, "checkpoint_timing.pt")
    t0 = time.perf_counter()
    upd.save_checkpoint(path)
    out["save_checkpoint_s"] = time.perf_counter() - t0
    out["file_bytes"] = os.path.getsize(path)
    from speecht5_amd import checkpoint
    t0 = time.perf_counter()
    checkpoint.load_checkpoint(path)
    out["load_checkpoint_s"] = time.perf_counter() - t0
    os.unlink(path)
    upd.close()
    if a.stats_csv and os.path.exists(a.stats_csv):
        rows = {}
        for r in csv.DictReader(open(a.stats_csv)):
            name = r.get("Name") or r.get("KernelName") or ""
            for key, moved in (("batch_load_kernel", 2 * sh_bytes), ("state_digest_kernel", sh_bytes + wflat_bytes), ("state_digest_finish_kernel", 0)):
                if key in name and (key != "state_digest_kernel" or "finish" not in name):
                    rows[key] = {"calls": int(r["Calls"]), "total_ns": float(r["TotalDurationNs"]), "max_ns": float(r["MaxNs"]),
                                 "min_ns": float(r["MinNs"])}
                    if moved:
                        # (the benched update has no source: the snapshot's is the only st5_batch_load of the traced run)
                        rows[key]["bytes"] = moved
                        rows[key]["GBps_at_max"] = moved / float(r["MaxNs"])
        out["snapshot"]["per_kernel"] = rows or "not measured (the kernels were not found in the statistics)"
    out["bench"] = "not measured (no --bench-json given)"
    if a.bench_json and os.path.exists(a.bench_json):
        out["bench"] = json.load(open(a.bench_json))
    txt = json.dumps(out, indent=1)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(txt + "\n")
    print(json.dumps({"update_ms": {k: {m: round(v[m], 3) for m in ("mean", "min", "max")} for k, v in out["update_ms"].items()},
                      "two_launches_ms": round(out["snapshot"]["two_launches_ms_by_events"]["median"], 3),
                      "copy_ms": round(out["snapshot"]["device_to_host_copy_ms_alone"]["median"], 2),
                      "save_checkpoint_s": round(out["save_checkpoint_s"], 2)}))


if __name__ == "__main__":
    main()
