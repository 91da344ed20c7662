"""Timing of the synthesis stream (generate_speech_stream) against batched synthesis (generate_speech_batch) on mixed text lengths.

Base size (t5_transformer_base, seeded random weights, every dropout 0), bf16, 64 texts whose seeded lengths are spread between 20 and
200 tokens; the stop bias is set to -20, so no stop probability reaches the threshold and every utterance runs to its maxlen (default
maxlenratio 20: 10 steps per token at reduction factor 2).  rows = 32, TTS_POLL_STEPS as the model has it, need_attn=False.  Arms,
alternated in one process after one warm-up call of each, whole calls on the host clock around a call that ends in a device
synchronise, every repeat kept:
  stream        generate_speech_stream(decode="graph") over the list in arrival order;
  batch         generate_speech_batch(decode="graph") over the same list in arrival order in batches of 32;
  batch_sorted  the same over the list sorted by length.
Reported per arm: utterances per second and total ticks (decode steps enqueued: device steps + graph replays).

Per-step cost: 32 texts of 100 tokens at threshold 2.0 (100 steps per row, the set-up of tools/tts_graph_timing.py, whose recorded
`steps_only_ms_per_step` of the "graph" arm at B = 32 is the scalar step of the commit before this one) through the stream's per-row
program and through the batch call's scalar program (also with key-padding bytes, which the stream's program always reads), HIP
events around every group of steps between two polls (tts_profile).

    python tools/tts_stream_timing.py [--reps 5] [--json profiles/tts_stream_timing.json]

--ops times every launch of the per-row step beside the same launch of the scalar step (profiles/tts_stream_ops.txt):

    python tools/tts_stream_timing.py --ops [--out profiles/tts_stream_ops.txt]

--count PROGRAM makes two calls of one step program in a fresh process for a kernel trace (profiles/tts_stream_kernel_stats_*.csv):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/tts_stream_timing.py --count per_row"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import functional as Fn  # noqa: E402
from speecht5_amd.tts_stream import stream_schedule  # noqa: E402
from tools.tts_batch_timing import build, texts, timed  # noqa: E402

ROWS, N_TEXTS, MIN_LEN, MAX_LEN, PAD = 32, 64, 20, 200, 1
PROFILE = {"step_ms": 0, "steps_timed": 0}      # of the last arm call, when the model's tts_profile is on


def requests(dev, seed=64):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(MIN_LEN, MAX_LEN + 1, (N_TEXTS,), generator=g).tolist()
    reqs = []
    for i, n in enumerate(lens):
        t = torch.randint(4, 81, (n,), generator=g)
        t[-1] = 2
        reqs.append((i, t.to(dev), torch.randn(512, generator=g).to(dev)))
    return reqs, lens


def batch_arm(model, reqs):
    """The list through generate_speech_batch in batches of ROWS (right-padded); returns ({key: mel frames}, ticks)."""
    frames, ticks = {}, 0
    PROFILE["step_ms"] = PROFILE["steps_timed"] = 0
    for i in range(0, len(reqs), ROWS):
        chunk = reqs[i:i + ROWS]
        toks = torch.full((len(chunk), max(q[1].numel() for q in chunk)), PAD, dtype=torch.long, device=chunk[0][1].device)
        for b, q in enumerate(chunk):
            toks[b, :q[1].numel()] = q[1]
        out = model.generate_speech_batch(src_tokens=toks, spkembs=torch.stack([q[2] for q in chunk]), need_attn=False, decode="graph")
        ticks += model.tts_device_steps + model.tts_graph_replays
        for k in PROFILE:
            PROFILE[k] += model.tts_stats.get(k, 0)
        for q, o in zip(chunk, out):
            frames[q[0]] = o[0].shape[0]
    return frames, ticks


def stream_arm(model, reqs):
    frames = {key: mel.shape[0] for key, mel, _, _ in model.generate_speech_stream(reqs, rows=ROWS, max_src_len=MAX_LEN, decode="graph")}
    for k in PROFILE:
        PROFILE[k] = model.tts_stats.get(k, 0)
    return frames, model.tts_device_steps + model.tts_graph_replays


def op_times(model, dev, out_path, n=200):
    """--ops: every launch of the per-row step program beside the same launch of the scalar program (32 rows, 100-token texts, both
    states 8 steps in): HIP events around n back-to-back launches of ONE op after 10 warm-up launches.  A kernel shorter than its
    launch shows the enqueue rate in both columns; what the table is for is the op whose two columns differ."""
    from speecht5_amd import tts_graph, tts_stream
    toks, spk = texts(ROWS, dev)
    enc, T_in = model._encode_rows(None, toks, None)
    sc = tts_graph.DeviceDecode(model, enc, T_in, spk, False, True, threshold=2.0)
    for _ in range(model.TTS_POLL_STEPS):
        sc.prog.step()
    stream = tts_stream.SynthesisStream(model, [(b, toks[b], spk[b]) for b in range(ROWS)], ROWS, toks.shape[1], "device", False, threshold=2.0)
    stream.advance()
    pr = stream.st
    assert len(sc.prog.ops) == len(pr.prog.ops)
    lines = ["# op index, builder | scalar us | per-row us | per-row - scalar"]
    total = [0.0, 0.0]
    for i, (a, b) in enumerate(zip(sc.prog.ops, pr.prog.ops)):
        us = []
        for fn in (a, b):
            for _ in range(10):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / n)
        total[0] += us[0]
        total[1] += us[1]
        lines.append(f"{i} {a.__qualname__.split('.<locals>')[0]} | {us[0]:.2f} | {us[1]:.2f} | {us[1] - us[0]:+.2f}")
        print(lines[-1], flush=True)
    lines.append(f"sum | {total[0]:.1f} | {total[1]:.1f} | {total[1] - total[0]:+.1f}")
    print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--ops", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--count", default=None, choices=["per_row", "scalar"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = build(dev, torch.bfloat16)
    if a.ops:
        with torch.no_grad():
            op_times(model, dev, a.out)
        return
    if a.count:
        # two calls of one step program in a fresh process, for a kernel trace:
        #   rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/tts_stream_timing.py --count per_row
        toks, spk = texts(ROWS, dev)
        with torch.no_grad():
            for _ in range(2):
                if a.count == "per_row":
                    list(model.generate_speech_stream([(b, toks[b], spk[b]) for b in range(ROWS)], rows=ROWS, max_src_len=toks.shape[1],
                                                      decode="graph", threshold=2.0))
                else:
                    model.generate_speech_batch(src_tokens=toks, spkembs=spk, threshold=2.0, need_attn=False, decode="graph")
            torch.cuda.synchronize()
        print(json.dumps(dict(mode="count", program=a.count, calls=2, replays_last_call=model.tts_graph_replays)))
        return
    with torch.no_grad():
        model.speech_decoder_postnet.prob_out.bias.fill_(-20.0)
    Fn.weight_cache.clear()
    r = model.reduction_factor
    reqs, lens = requests(dev)
    by_len = sorted(reqs, key=lambda q: q[1].numel())
    steps = [int(n * 20.0 / r) for n in lens]
    arms = {"stream": lambda: stream_arm(model, reqs), "batch": lambda: batch_arm(model, reqs),
            "batch_sorted": lambda: batch_arm(model, by_len)}
    results, times, ticks = [], {k: [] for k in arms}, {}
    with torch.no_grad():
        for name, fn in arms.items():                      # warm-up, and every arm gives every utterance its maxlen
            _, (frames, ticks[name]) = timed(fn)
            assert frames == {i: s * r for i, s in enumerate(steps)}, name
        assert ticks["stream"] == stream_schedule(steps, ROWS, model.TTS_POLL_STEPS)[0]
        for rep in range(a.reps):
            for name, fn in arms.items():
                dt, (_, t) = timed(fn)
                assert t == ticks[name]
                times[name].append(dt)
            print(f"# repeat {rep + 1}: " + ", ".join(f"{k} {v[-1]:.4f} s" for k, v in times.items()), flush=True)
        # where a call's time goes: one more call of each arm with HIP events around every group of steps between two polls
        inside = {}
        model.tts_profile = True
        try:
            for name, fn in arms.items():
                dt, _ = timed(fn)
                inside[name] = dict(profiled_call_s=round(dt, 5), steps_only_s=round(PROFILE["step_ms"] * 1e-3, 5),
                                    steps_only_ms_per_tick=round(PROFILE["step_ms"] / max(PROFILE["steps_timed"], 1), 4))
        finally:
            model.tts_profile = False
        for name in arms:
            med = statistics.median(times[name])
            results.append(dict(kind="throughput", arm=name, dtype="bf16", texts=N_TEXTS, rows=ROWS, lengths_tokens=[min(lens), max(lens)],
                                sum_steps=sum(steps), max_steps=max(steps), poll_steps=model.TTS_POLL_STEPS, ticks=ticks[name],
                                utt_per_s=round(N_TEXTS / med, 3), call_s=[round(t, 5) for t in times[name]], call_s_median=round(med, 5),
                                ms_per_tick=round(med / ticks[name] * 1e3, 4), **inside[name]))
            print(json.dumps(results[-1]), flush=True)

        # ---- per-step cost: the per-row program against the scalar program at the same 32 rows, 100 steps each ----
        toks, spk = texts(ROWS, dev)
        same = [(b, toks[b], spk[b]) for b in range(ROWS)]
        padded = toks.clone()
        padded[0, -1] = PAD
        progs = {"per_row": lambda: list(model.generate_speech_stream(same, rows=ROWS, max_src_len=toks.shape[1], decode="graph", threshold=2.0)),
                 "scalar": lambda: model.generate_speech_batch(src_tokens=toks, spkembs=spk, threshold=2.0, need_attn=False, decode="graph"),
                 # the scalar program with key-padding bytes, which the stream's program always reads: row 0 one token shorter
                 "scalar_kpm": lambda: model.generate_speech_batch(src_tokens=padded, spkembs=spk, threshold=2.0, need_attn=False,
                                                                   decode="graph")}
        per_step, timed_n = {k: [] for k in progs}, {}
        model.tts_profile = True
        try:
            for name, fn in progs.items():
                timed(fn)
            for _ in range(a.reps):
                for name, fn in progs.items():
                    timed(fn)
                    st = model.tts_stats
                    per_step[name].append(st["step_ms"] / st["steps_timed"])
                    timed_n[name] = st["steps_timed"]
        finally:
            model.tts_profile = False
        for name, v in per_step.items():
            results.append(dict(kind="step", program=name, dtype="bf16", rows=ROWS, steps_timed=timed_n[name],
                                steps_only_ms_per_step=[round(x, 4) for x in v], median=round(statistics.median(v), 4)))
            print(json.dumps(results[-1]), flush=True)
    Fn.set_compute_dtype(torch.float32)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
