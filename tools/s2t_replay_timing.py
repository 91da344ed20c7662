"""What replaying the ASR fine-tuning update buys (update.PretrainUpdate on an s2t micro-batch): Base
t5_transformer_base_asr, bf16, 8 x 10 s of speech with targets of 200 labels through collate.SpeechToTextCollater(fixed_shape=...),
CE + CTC (0.5 / 0.5), sentence_avg, one micro-batch in turn, one GPU, encoder not frozen.

update  two arms ALTERNATED in one process on the same model weights, seeds and batches (a source cycling over two batches), after three
        warm-up updates of each; one repeat = `--updates` updates between two device synchronisations, host clock, ms per update; every
        repeat is kept:
          eager     PretrainUpdate(graph=False) with the criterion's defaults (device_targets=False: masked_select and its host read,
                    the channel mask as an eager copy) -- the launches the parent commit issues for this update
          replayed  PretrainUpdate(graph=True, prefetch_host=True), criterion device_targets=True: the captured step
pack    the st5_ctc_pack_rows launch alone at B = 8, L = 201 (it reads and writes 2 * B * L * 8 bytes), after a warm-up: HIP events
        around single calls of functional.ctc_pack_rows on an otherwise idle stream and around groups of ten (per call = group / 10)
        -- these include the call's host side, two allocations and the ctypes call -- and around replays of a captured chain of 100
        launches into preallocated outputs (per launch = replay / 100): the launch as a node of a captured step.

    python tools/s2t_replay_timing.py [--reps 5] [--updates 20] [--json profiles/s2t_replay_timing.json] [--commits parent,this]"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import functional as Fn  # noqa: E402

B, SECONDS, LABELS = 8, 10, 200


def summary(v):
    return {"mean": statistics.mean(v), "median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "all": v}


def build(dev):
    from speecht5_amd.speecht5 import t5_transformer_base_asr
    from speecht5_amd.task import SpeechT5Task
    Fn.set_compute_dtype(torch.bfloat16)
    args = Namespace(label_rates=50, sample_rate=16000, speech_odim=80, bert_init=True, share_input_output_embed=True)
    t5_transformer_base_asr(args)
    task = SpeechT5Task.synthetic(args)
    torch.manual_seed(1337)
    model = task.build_model(args).to(dev).train()
    return args, task, model


def batches(dev, task, n):
    from speecht5_amd.collate import SpeechToTextCollater
    d = task.target_dictionary
    coll = SpeechToTextCollater(dev, pad_idx=d.pad(), eos_idx=d.eos(), fixed_shape=(SECONDS * 16000, LABELS + 1))
    g = torch.Generator().manual_seed(99)
    hi = d.index("<mask>")      # labels are characters: below the two symbols the task appends
    out = []
    for k in range(n):
        items = [{"id": k * B + i, "source": torch.randn(SECONDS * 16000, generator=g).to(dev),
                  "label_list": [torch.randint(4, hi, (LABELS,), generator=g).to(dev)]} for i in range(B)]
        out.append([coll(items)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--commits", default="")
    a = ap.parse_args()
    from speecht5_amd.criterions import SpeechtoTextLoss
    from speecht5_amd.update import PretrainUpdate
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arms = {}
    for name in ("eager", "replayed"):
        args, task, model = build(dev)
        crit = SpeechtoTextLoss(SimpleNamespace(zero_infinity=True), task, sentence_avg=True, label_smoothing=0.1, report_accuracy=True,
                                ce_weight=0.5, ctc_weight=0.5, sync_logging=False, device_targets=name == "replayed")
        data = batches(dev, task, 3)
        Fn.manual_seed(21)
        np.random.seed(8)
        torch.manual_seed(8)
        upd = PretrainUpdate(task, model, crit, data[0], lr=1e-4, clip_norm=1.0, graph=name == "replayed", micro="in_turn",
                             prefetch_host=True, device=dev, stats=True)
        upd.set_source(itertools.cycle(data[1:]))
        if name == "replayed":
            upd.prepare_graph()
        arms[name] = upd
    for upd in arms.values():
        for _ in range(3):
            upd.update()
        upd.finish()
        upd.logging_outputs()
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
            upd.logging_outputs()
    out = {"shape": f"t5_transformer_base_asr bf16, {B} x {SECONDS} s, {LABELS} labels per target, CE + CTC, in_turn, one micro-batch",
           "gpu": torch.cuda.get_device_name(dev), "updates_per_repeat": a.updates, "commits": a.commits,
           "update_ms": {k: summary(v) for k, v in times.items()}}

    # ---- the pack launch alone ----
    d = arms["replayed"].task.target_dictionary
    target = arms["replayed"].micro[0]["target"]
    torch.cuda.synchronize()

    def events(n, group):
        res = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(group):
                Fn.ctc_pack_rows(target, d.pad(), d.eos())
            e1.record()
            torch.cuda.synchronize()
            res.append(e0.elapsed_time(e1) * 1e3 / group)
        return res
    events(5, 1)

    def chained(n_launch, reps):
        """n_launch launches through the C ABI into preallocated outputs, captured as one chain of kernel nodes and replayed: per
        launch = replay / n_launch -- the device's side of a launch inside a captured step, no host work in between."""
        from speecht5_amd import hip
        Bt, Lt = target.shape
        packed, meta = torch.empty_like(target), torch.empty(2 * Bt + 1, dtype=torch.int64, device=dev)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            for _ in range(n_launch):
                hip.check(hip.lib().st5_ctc_pack_rows(target.data_ptr(), d.pad(), d.eos(), Bt, Lt, packed.data_ptr(), meta.data_ptr(),
                                                      meta.data_ptr() + 8 * Bt, meta.data_ptr() + 16 * Bt, hip.stream()), "st5_ctc_pack_rows")
        g.replay()
        torch.cuda.synchronize()
        res = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            res.append(e0.elapsed_time(e1) * 1e3 / n_launch)
        return res
    # single / group: events around Fn.ctc_pack_rows on an idle stream -- these include the call's host side (two allocations, the
    # ctypes call); chain_of_100: the launch as a node of a captured chain
    out["pack_us"] = {"B": int(target.shape[0]), "L": int(target.shape[1]), "bytes": 2 * target.numel() * 8,
                      "single_us": summary(events(max(a.reps, 7) * 3, 1)), "group_of_10_us_per_launch": summary(events(max(a.reps, 7), 10)),
                      "chain_of_100_us_per_launch": summary(chained(100, max(a.reps, 7)))}
    for upd in arms.values():
        upd.close()
    txt = json.dumps(out, indent=1)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(txt + "\n")
    print(json.dumps({"update_ms": {k: {m: round(v[m], 3) for m in ("mean", "min", "max")} for k, v in out["update_ms"].items()},
                      "pack_us": round(out["pack_us"]["single_us"]["median"], 2),
                      "pack_us_in_group": round(out["pack_us"]["group_of_10_us_per_launch"]["median"], 2),
                      "pack_us_in_chain": round(out["pack_us"]["chain_of_100_us_per_launch"]["median"], 2)}))


if __name__ == "__main__":
    main()
