"""Timing of the graph-replayed TTS decode (generate_speech_batch(decode=...)) against the eager batched decode.

Base size (t5_transformer_base, seeded random weights, every dropout 0), 100-token texts, threshold = 2.0 (exactly 100 decode steps per
row), need_attn=False, fp32 and bf16, B in {1, 8, 32}.  Three arms -- decode="eager", "device", "graph" -- alternated inside one process
after a warm-up call of each; whole calls are timed (encoder, set-up and, for "graph", the capture included; host clock around a call
that ends in a device synchronise).  Every repeat is kept.  Three further calls of "device" and "graph" time the steps alone (HIP events
around every group of steps between two polls: `steps_only_ms_per_step`) and the capture (`capture_ms`, host clock).

    python tools/tts_graph_timing.py [--B 1 8 32] [--dtype bf16 fp32] [--reps 5] [--json profiles/tts_graph_timing.json]

--shapes times st5_gemm_skinny against st5_gemm per (N, K) of the decode step (and of the shallow-fusion LM) at M in {1, 8, 32} with HIP
events around 200 back-to-back launches after 20 warm-up launches, and reports microseconds per launch and weight bytes per second.
Both arms write into a preallocated output from a prepared weight image (Fn.linear_skinny / hip.gemm), so their host paths are alike;
what the events see is still the enqueue rate wherever a kernel is shorter than its launch (~5 us per launch here):

    python tools/tts_graph_timing.py --shapes [--out profiles/decode_gemm_shapes.txt]

--count ARM makes two calls of one arm in a fresh process for a kernel trace (launches per step: the difference between a trace at
--count-threshold 2.0, 100 steps, and one at 1.0, 50 steps, over the 2 x 50 steps):

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/tts_graph_timing.py --count graph --B 8 --dtype bf16"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import functional as Fn  # noqa: E402
from tools.tts_batch_timing import STEPS, build, texts, timed  # noqa: E402

ARMS = ["eager", "device", "graph"]
SHAPES = [(256, 80), (256, 256), (768, 256), (768, 1280), (768, 768), (1536, 768), (2304, 768), (3072, 768), (768, 3072), (162, 768),
          (1280, 1280), (3840, 1280), (6144, 1280), (1280, 6144)]


def arm_fn(model, arm, toks, spk, threshold):
    return lambda: model.generate_speech_batch(src_tokens=toks, spkembs=spk, threshold=threshold, need_attn=False, decode=arm)


def shape_times(dev, out_path):
    lines = ["# dtype N K M | st5_gemm_skinny us, weight GB/s | st5_gemm us, weight GB/s | skinny / st5_gemm"]
    for dname, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        Fn.set_compute_dtype(dtype)
        for N, K in SHAPES:
            w32 = torch.randn(N, K, device=dev) / K ** 0.5
            b = torch.randn(N, device=dev)
            w = w32.to(dtype)
            ws = Fn.gemm_skinny_ws(N, K, dev)
            for M in (1, 8, 32):
                x = torch.randn(M, K, device=dev).to(dtype)
                out = torch.empty(M, N, dtype=dtype, device=dev)
                from speecht5_amd import hip
                out2 = torch.empty(M, (N + 7) // 8 * 8, dtype=dtype, device=dev)
                A, Bw, Cc = hip.operand(x, K), hip.operand(w, K), hip.operand(out2, out2.shape[1])
                fns = {"skinny": lambda: Fn.linear_skinny(x, w, b, out=out, ws=ws),
                       "st5_gemm": lambda: hip.gemm(A, Bw, Cc, M, N, K, hip.dt(dtype), bias=b)}
                us = {}
                for name, fn in fns.items():
                    for _ in range(20):
                        fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(200):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    us[name] = e0.elapsed_time(e1) * 1e3 / 200
                wb = N * K * w.element_size()
                lines.append(f"{dname} {N} {K} {M} | {us['skinny']:.2f} us, {wb / us['skinny'] * 1e-3:.1f} GB/s | {us['st5_gemm']:.2f} us, "
                             f"{wb / us['st5_gemm'] * 1e-3:.1f} GB/s | {us['skinny'] / us['st5_gemm']:.2f}")
                print(lines[-1], flush=True)
            Fn.weight_cache.clear()
    Fn.set_compute_dtype(torch.float32)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--dtype", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", default=None, choices=ARMS)
    ap.add_argument("--count-threshold", type=float, default=2.0)
    ap.add_argument("--shapes", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.shapes:
        with torch.no_grad():
            shape_times(dev, a.out)
        return
    results = []
    for dname in a.dtype:
        dtype = torch.float32 if dname == "fp32" else torch.bfloat16
        model = build(dev, dtype)
        with torch.no_grad():
            if a.count:
                toks, spk = texts(a.B[0], dev)
                for _ in range(2):
                    timed(arm_fn(model, a.count, toks, spk, a.count_threshold))
                print(json.dumps(dict(mode="count", arm=a.count, B=a.B[0], dtype=dname, calls=2, threshold=a.count_threshold,
                                      replays_last_call=model.tts_graph_replays)))
                continue
            for B in a.B:
                toks, spk = texts(B, dev)
                fns = {arm: arm_fn(model, arm, toks, spk, 2.0) for arm in ARMS}
                for arm in ARMS:                              # warm-up
                    _, out = timed(fns[arm])
                    lens = [o[0].shape[0] // model.reduction_factor for o in out]
                    assert lens == [STEPS] * B and model.tts_decode_mode == arm, (arm, lens)
                times = {arm: [] for arm in ARMS}
                extra = {}
                for _ in range(a.reps):
                    for arm in ARMS:
                        dt, _ = timed(fns[arm])
                        times[arm].append(dt)
                        extra[arm] = dict(host_polls_per_call=model.tts_polls, graph_replays_per_call=model.tts_graph_replays)
                    print(f"# {dname} B={B} repeat {len(times['eager'])}: " + ", ".join(f"{k} {v[-1]:.4f} s" for k, v in times.items()),
                          flush=True)
                # the steps apart from set-up and capture: three more calls of the new arms with HIP events around every group of
                # steps between two polls (device time from a group's first launch to the end of its last kernel; the host waits at
                # every poll, so the groups do not overlap), and the host time of the capture
                inside = {}
                model.tts_profile = True
                try:
                    for arm in ARMS[1:]:
                        per_step, capture = [], []
                        for _ in range(3):
                            timed(fns[arm])
                            st = model.tts_stats
                            per_step.append(st["step_ms"] / st["steps_timed"])
                            capture.append(st.get("capture_s", 0.0) * 1e3)
                        inside[arm] = dict(steps_only_ms_per_step=[round(v, 4) for v in per_step],
                                           capture_ms=[round(v, 2) for v in capture], steps_timed=st["steps_timed"])
                finally:
                    model.tts_profile = False
                med_eager = statistics.median(times["eager"])
                for arm in ARMS:
                    ts = times[arm]
                    med = statistics.median(ts)
                    r = dict(dtype=dname, B=B, arm=arm, utt_per_s=round(B / med, 3), ms_per_step=round(med / STEPS * 1e3, 4),
                             call_s=[round(t, 5) for t in ts], call_s_median=round(med, 5), speedup_vs_eager=round(med_eager / med, 3),
                             every_repeat_faster_than_every_eager=bool(max(ts) < min(times["eager"])), decode_steps_per_call=STEPS, **extra[arm], **inside.get(arm, {}))
                    results.append(r)
                    print(json.dumps(r), flush=True)
        del model
        torch.cuda.empty_cache()
    Fn.set_compute_dtype(torch.float32)
    if a.json and results:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
