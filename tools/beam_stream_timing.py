"""Timing of the beam-search stream (SequenceGenerator.generate_stream) against batched generate(decode="graph", exact_rows=True) on
mixed clip lengths.

Base size (t5_transformer_base, seeded random weights, eval), bf16, the 83-entry character dictionary of the ASR recipe, 64 seeded
clips of 2 to 20 s in a fixed shuffled arrival order.  The step limit of a sentence is proportional to its duration (max_len_a =
STEPS_PER_SECOND / 16000, max_len_b = 0) and every sentence runs to its limit: the final LayerNorm's bias gets +30 in channel 0 and
the tied embedding's eos row becomes -5 in that channel and 0 elsewhere, so eos is ~150 below every other logit until the limit forces
it.  In a batch call the limit is the formula on the PADDED length, so every sentence of a batch runs to the longest one's limit --
that is what keeping finished sentences in the batch costs, and it is also why the arms' hypotheses are not the same texts.
Configurations: beam 5 with 6 slots, beam 10 with 3 slots.  Arms, alternated in one process after one warm-up call of each, whole
calls on the host clock around a call that ends in a device synchronise, every repeat kept:
  stream        generate_stream(decode="graph") over the list in arrival order;
  batch         generate(decode="graph", exact_rows=True) over the same list in arrival order in batches of the slot count;
  batch_sorted  the same over the list sorted by length.
Reported per arm: sentences per second and total steps (device steps + graph replays); for the stream also the per-poll overhead:
(whole call - device time of the steps) / polls, which holds the admissions, the encoder work and the host's part.

Per-step cost: `slots` clips of 10 s through the stream's per-sentence program and through the scalar program of beam_graph.py (the
parent commit's step, unchanged) at the same rows and limits, HIP events around every group of steps between two polls.

--joint-ctc: the same workload and arms with joint CTC / attention scoring (ctc_weight 0.5, ctc_rows=True): the stream is
generate_stream(joint_ctc=True), the batch arms are generate(decode="graph", ctc_rows=True), the per-step comparison is the per-slot
CTC step against the scalar CTC step of beam_graph.py at the same rows.  A random model's next-token distribution is nearly flat, and
under a flat distribution a hypothesis soon leaves its 7 x beam CTC candidates (tools/beam_ctc_timing.py); --temperature (the same
for every arm) sharpens it, the values are tried in order and the first under which no arm raises the generator's KeyError is
measured and recorded with the ones that raised; a configuration under which every temperature raises is reported and the tool exits
non-zero.

--lm (combinable with --joint-ctc): the same workload and arms with Transformer-LM shallow fusion: a seeded random LM of the
transformer_lm_t5 preset as tools/beam_lm_timing.py builds it (20 layers x 1280, FFN 6144, 16 heads, 83 symbols), lm_weight 0.3.  The
stream is generate_stream of a generator built with that lm_model, the batch arms are generate(decode="graph", exact_rows=True,
lm_model=...), the per-step comparison is the per-slot LM step (TransformerLanguageModel.device_step_sents,
st5_beam_lm_logprobs_sents) against the scalar LM step of beam_graph.py (the parent commit's step, unchanged) at the same rows and
limits.  The LM's term (0.3 x a nearly flat log-softmax) is far below the ~150 that keep eos away, so every sentence still runs to its
limit.

    python tools/beam_stream_timing.py [--reps 5] [--json profiles/beam_stream_timing.json]
    python tools/beam_stream_timing.py --joint-ctc [--temperature 0.25 0.05] [--json profiles/beam_stream_ctc_timing.json]
    python tools/beam_stream_timing.py --lm [--json profiles/beam_stream_lm_timing.json]
    python tools/beam_stream_timing.py --lm --joint-ctc [--json profiles/beam_stream_ctc_lm_timing.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import beam_graph  # noqa: E402
from speecht5_amd import functional as Fn  # noqa: E402
from speecht5_amd.step_program import on_decode_stream, run_steps  # noqa: E402
from speecht5_amd.tts_stream import stream_schedule  # noqa: E402
from beam_lm_timing import LM_WEIGHT, build_lm  # noqa: E402
from beam_slots_timing import build_model, timed  # noqa: E402
from speech_rows_timing import RATE, batch  # noqa: E402

N_CLIPS, MIN_S, MAX_S, STEPS_PER_SECOND = 64, 2, 20, 5
CONFIGS = [(5, 6), (10, 3)]          # (beam, slots)


def suppress_eos(model, d):
    dec = model.decoder
    ln = dec.layer_norm if dec.layer_norm is not None else dec.layers[-1].final_layer_norm
    with torch.no_grad():
        ln.bias[0] += 30.0
        row = model.text_decoder_prenet.embed_tokens.weight[d.eos()]
        row.zero_()
        row[0] = -5.0
    Fn.weight_cache.clear()


def clips(dev, seed=64):
    g = torch.Generator().manual_seed(seed)
    n = (torch.randint(MIN_S * 10, MAX_S * 10 + 1, (N_CLIPS,), generator=g) * (RATE // 10)).tolist()      # arrival order: shuffled
    wav, _ = batch(n, dev, seed=seed)
    return [(i, wav[i, :m].clone()) for i, m in enumerate(n)], n


CTC_WEIGHT = 0.5


def generator(model, d, beam, decode="concat", joint_ctc=False, temperature=1.0, lm=None):
    from speecht5_amd.sequence_generator import SequenceGenerator
    ctc = dict(ctc_weight=CTC_WEIGHT, ctc_rows=True, temperature=temperature) if joint_ctc else {}
    fuse = dict(lm_model=lm, lm_weight=LM_WEIGHT) if lm is not None else {}
    return SequenceGenerator([model], d, beam_size=beam, max_len_a=STEPS_PER_SECOND / RATE, max_len_b=0, exact_rows=True, decode=decode,
                             **ctc, **fuse)


def stream_arm(gen, reqs, slots):
    kw = dict(joint_ctc=True) if gen.ctc_weight > 0 else {}
    n = sum(1 for _ in gen.generate_stream(reqs, sentences=slots, max_src_len=MAX_S * RATE, decode="graph", **kw))
    assert n == len(reqs)
    st = gen.beam_stream_stats
    return gen.beam_device_steps + gen.beam_graph_replays, gen.beam_polls, st.get("step_ms", 0.0), st.get("steps_timed", 0), dict(st["sentence_steps"])


def batch_arm(gen, reqs, slots):
    steps = polls = 0
    for i in range(0, len(reqs), slots):
        chunk = reqs[i:i + slots]
        m = max(w.numel() for _, w in chunk)
        wav = torch.zeros(len(chunk), m, device=chunk[0][1].device)
        pad = torch.ones(len(chunk), m, dtype=torch.bool, device=wav.device)
        for b, (_, w) in enumerate(chunk):
            wav[b, :w.numel()] = w
            pad[b, :w.numel()] = False
        out = gen.generate(None, {"net_input": {"source": wav, "padding_mask": pad}})
        assert len(out) == len(chunk)
        steps += gen.beam_device_steps + gen.beam_graph_replays
        polls += gen.beam_polls
    return steps, polls, 0.0, 0, None


def scalar_steps(gen, model, sample, n_sent):
    """The scalar step program of beam_graph.py on one batch, HIP events around every group of steps: (ms, steps timed)."""
    net_input = sample["net_input"]
    src_len = net_input["source"].size(1)
    max_len = min(int(gen.max_len_a * src_len + gen.max_len_b), gen.max_len - 1)
    enc = gen.model.forward_encoder(net_input, exact_rows=True)
    stats = {"polls": 0, "device_steps": 0, "graph_replays": 0}
    with on_decode_stream(model, net_input["source"].device, "graph"):
        st = beam_graph.BeamDeviceDecode(gen, model, enc[0], n_sent, max_len, gen.eos)
        run_steps(st.prog.step, max_len + 1, "graph", gen.BEAM_POLL_STEPS, lambda: st.poll() == n_sent, stats, profile=True)
    torch.cuda.synchronize()
    return stats["step_ms"], stats["steps_timed"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--joint-ctc", action="store_true")
    ap.add_argument("--lm", action="store_true", help="Transformer-LM shallow fusion (transformer_lm_t5 preset, lm_weight 0.3)")
    ap.add_argument("--temperature", type=float, nargs="+", default=[0.25, 0.05])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model, d = build_model(dev, torch.bfloat16)
    assert len(d) == 83
    suppress_eos(model, d)
    lm = build_lm(dev, len(d)) if a.lm else None
    reqs, n = clips(dev)
    by_len = sorted(reqs, key=lambda q: q[1].numel())
    limits = [int(STEPS_PER_SECOND / RATE * m) for m in n]
    results, failed = [], []
    with torch.no_grad():
        for beam, slots in CONFIGS:
            raised = []
            for temperature in (a.temperature if a.joint_ctc else [1.0]):
                try:
                    part = measure_config(a, dev, model, d, reqs, by_len, n, limits, beam, slots, temperature, lm)
                except KeyError as e:
                    torch.cuda.synchronize()
                    raised.append(temperature)
                    print(f"# beam {beam} x {slots}, temperature {temperature}: {str(e)[:200]}", flush=True)
                    continue
                for r in part:
                    if a.joint_ctc:
                        r.update(ctc_weight=CTC_WEIGHT, ctc_rows=True, temperature=temperature, key_error_at_temperature=raised)
                    if a.lm:
                        r.update(lm="transformer_lm_t5", lm_weight=LM_WEIGHT)
                    print(json.dumps(r), flush=True)
                results.extend(part)
                break
            else:
                failed.append((beam, slots))
                results.append(dict(kind="not_measured", beam=beam, slots=slots, ctc_weight=CTC_WEIGHT, key_error_at_temperature=raised))
            if a.json:
                with open(a.json, "w") as f:
                    json.dump(results, f, indent=1)
    Fn.set_compute_dtype(torch.float32)
    if failed:
        sys.exit(f"beam_stream_timing: no timing for (beam, slots) {failed}: every temperature raised the CTC KeyError")


def measure_config(a, dev, model, d, reqs, by_len, n, limits, beam, slots, temperature, lm=None):
    """The result rows of one (beam, slots) configuration.  KeyError (joint CTC only): a hypothesis left its CTC candidates."""
    results = []
    gs = generator(model, d, beam, joint_ctc=a.joint_ctc, temperature=temperature, lm=lm)
    gb = generator(model, d, beam, "graph", joint_ctc=a.joint_ctc, temperature=temperature, lm=lm)
    P = gs.BEAM_POLL_STEPS
    arms = {"stream": lambda: stream_arm(gs, reqs, slots), "batch": lambda: batch_arm(gb, reqs, slots),
            "batch_sorted": lambda: batch_arm(gb, by_len, slots)}
    steps, polls, times = {}, {}, {k: [] for k in arms}
    for name, fn in arms.items():                  # warm-up; every sentence of the stream runs to its own limit
        _, (steps[name], polls[name], _, _, per_sentence) = timed(fn)
        if per_sentence is not None:
            assert per_sentence == {i: m + 1 for i, m in enumerate(limits)}, "a sentence ended before its limit"
    assert steps["stream"] == stream_schedule([m + 1 for m in limits], slots, P)[0]
    for rep in range(a.reps):
        for name, fn in arms.items():
            dt, out = timed(fn)
            assert out[0] == steps[name]
            times[name].append(dt)
        print(f"# beam {beam} x {slots}, repeat {rep + 1}: " + ", ".join(f"{k} {v[-1]:.4f} s" for k, v in times.items()), flush=True)
    gs.beam_profile = True                         # one more stream call with HIP events around every group of steps
    try:
        dt, (_, _, step_ms, timed_n, _) = timed(arms["stream"])
    finally:
        gs.beam_profile = False
    for name in arms:
        med = statistics.median(times[name])
        r = dict(kind="throughput", arm=name, dtype="bf16", beam=beam, slots=slots, clips=N_CLIPS, seconds=[min(n) // RATE, max(n) // RATE],
                 sum_steps=sum(m + 1 for m in limits), poll_steps=P, steps=steps[name], polls=polls[name],
                 sentences_per_s=round(N_CLIPS / med, 3), call_s=[round(t, 4) for t in times[name]], call_s_median=round(med, 4),
                 ms_per_step=round(med / steps[name] * 1e3, 4))
        if name == "stream":
            r.update(profiled_call_s=round(dt, 4), steps_only_s=round(step_ms * 1e-3, 4),
                     steps_only_ms_per_step=round(step_ms / max(timed_n, 1), 4),
                     overhead_ms_per_poll=round((dt - step_ms * 1e-3) / max(polls[name], 1) * 1e3, 4))
        results.append(r)

    # ---- per-step cost: the per-sentence program against the scalar program, `slots` clips of 10 s, the same rows ----
    wav, pad = batch([10 * RATE] * slots, dev, seed=7)
    same = [(b, wav[b]) for b in range(slots)]
    sample = {"net_input": {"source": wav, "padding_mask": pad}}
    per = {"per_sentence": [], "scalar": []}
    timed_n = {}
    gs.beam_profile = True
    try:
        for rep in range(a.reps + 1):              # (the first round is the warm-up)
            list(gs.generate_stream(same, sentences=slots, max_src_len=10 * RATE, decode="graph",
                                    **(dict(joint_ctc=True) if a.joint_ctc else {})))
            st = gs.beam_stream_stats
            ms, k = scalar_steps(gb, model, sample, slots)
            if rep:
                per["per_sentence"].append(st["step_ms"] / st["steps_timed"])
                per["scalar"].append(ms / k)
                timed_n = {"per_sentence": st["steps_timed"], "scalar": k}
    finally:
        gs.beam_profile = False
    for name, v in per.items():
        results.append(dict(kind="step", program=name, dtype="bf16", beam=beam, slots=slots, rows=beam * slots, S=499,
                            steps_timed=timed_n[name], steps_only_ms_per_step=[round(x, 4) for x in v],
                            median=round(statistics.median(v), 4)))
    return results


if __name__ == "__main__":
    main()
