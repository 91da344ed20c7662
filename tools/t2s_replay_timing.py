"""What a fixed shape costs and what replaying buys for TTS fine-tuning (update.PretrainUpdate on a t2s micro-batch):
t5_transformer_base, bf16, the batch and shape of tools/bench_cfg3.py (32 texts, fixed shape 100 tokens x 600 mel frames, reduction
factor 2, guided-attention loss, dropout 0.15), utterance and text lengths drawn between half and all of the fixed shape, one
micro-batch in turn, one GPU, statistics ring on.

update  three arms ALTERNATED in one process on the same model weights, seeds and utterances (a source cycling over four batches),
        after three warm-up updates of each; one repeat = `--updates` updates between two device synchronisations, host clock, ms per
        update; every repeat is kept:
          eager_own     PretrainUpdate(graph=False) on collate.TextToSpeechCollater() batches: every batch at its own lengths -- the
                        launches the parent commit issues for this update
          eager_fixed   PretrainUpdate(graph=False) on TextToSpeechCollater(fixed_shape=(100, 600)) batches: the price of the padding
                        (and of the live-frame post-net kernels) without the replay
          replayed      PretrainUpdate(graph=True, prefetch_host=True) on the same fixed-shape batches, criterion device_ntokens=True
bn      st5_batchnorm_act_fwd_live + _bwd_live against st5_batchnorm_act_fwd + _bwd at *live == Lx, at the post-net's shape in this
        batch ([32 * 600, postnet_chans] fp32 in, haloed bf16 out, tanh, dropout 0.5): HIP events around groups of 20 forward + backward
        pairs through the C ABI, the two alternated, us per pair.

    python tools/t2s_replay_timing.py [--reps 5] [--updates 20] [--json profiles/t2s_replay_timing.json] [--commits parent,this]"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import functional as Fn  # noqa: E402

B, TOKENS, FRAMES, R = 32, 100, 600, 2
ARMS = ("eager_own", "eager_fixed", "replayed")


def summary(v):
    return {"mean": statistics.mean(v), "median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "all": v}


def build(dev):
    from speecht5_amd.speecht5 import t5_transformer_base
    from speecht5_amd.task import SpeechT5Task
    Fn.set_compute_dtype(torch.bfloat16)
    args = Namespace(label_rates=50, sample_rate=16000, speech_odim=80, bert_init=True, use_codebook=False, share_input_output_embed=True,
                     encoder_layerdrop=0.0, decoder_layerdrop=0.0, dropout=0.15, attention_dropout=0.15, activation_dropout=0.15)
    t5_transformer_base(args)
    assert args.reduction_factor == R
    task = SpeechT5Task.synthetic(args)
    task.t5_task = "t2s"
    torch.manual_seed(1337)
    model = task.build_model(args).to(dev).train()
    return args, task, model


def batches(dev, task, args, n, fixed):
    """n batches of B synthetic utterances, lengths between half and all of the fixed shape (the same utterances for every arm)."""
    from speecht5_amd.collate import TextToSpeechCollater
    d = task.dicts["text"]
    coll = TextToSpeechCollater(dev, pad_idx=d.pad(), reduction_factor=R, fixed_shape=(TOKENS, FRAMES) if fixed else None)
    g = torch.Generator().manual_seed(99)
    out, lens = [], []
    for k in range(n):
        nf = torch.randint(FRAMES // 2, FRAMES + 1, (B,), generator=g).tolist()
        nt = torch.randint(TOKENS // 2, TOKENS + 1, (B,), generator=g).tolist()
        items = [{"id": k * B + i, "source": [torch.cat([torch.randint(4, len(d) - 2, (nt[i] - 1,), generator=g), torch.tensor([d.eos()])]).to(dev)],
                  "target": (torch.randn(nf[i], 80, generator=g) * 0.5 - 1).to(dev),
                  "spkembs": torch.randn(args.spk_embed_dim, generator=g).to(dev)} for i in range(B)]
        out.append([coll(items)])
        lens.append({"frames_max": max(nf), "frames_mean": sum(nf) / B, "tokens_max": max(nt), "tokens_mean": sum(nt) / B})
    return out, lens


def bn_pairs(dev, C, reps, group=20):
    """us per forward + backward pair of the existing and of the live BatchNorm entry points at *live == Lx, alternated."""
    from speecht5_amd import hip
    L = hip.lib()
    rows, Lx, pad = B * FRAMES, FRAMES, 2
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn(rows, C, generator=g).to(dev), torch.randn(rows, C, generator=g).to(dev)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    rm, rv, nbt = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    y = torch.empty(B, Lx + 2 * pad, C, dtype=torch.bfloat16, device=dev)
    dx = torch.empty_like(y)
    stats, dg, db = torch.empty(2 * C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    ws = hip.workspace(L.st5_batchnorm_ws_bytes(C), dev)
    live = torch.tensor([Lx], dtype=torch.int32, device=dev)
    omap = (Lx, (Lx + 2 * pad) * C, pad * C, pad)
    fwd = (x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), 0.1, 1e-5, 1, hip.ACT_TANH, 0.5, 77,
           0, y.data_ptr(), 0, stats.data_ptr(), ws.data_ptr(), rows, C, *omap)
    bwd = (x.data_ptr(), dy.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dg.data_ptr(), db.data_ptr(), 1, hip.ACT_TANH, 0.5,
           77, dx.data_ptr(), ws.data_ptr(), rows, C, *omap)
    tail = (hip.dt(torch.bfloat16), hip.stream())

    def pair(is_live):
        if is_live:
            hip.check(L.st5_batchnorm_act_fwd_live(*fwd, live.data_ptr(), Lx, *tail), "st5_batchnorm_act_fwd_live")
            hip.check(L.st5_batchnorm_act_bwd_live(*bwd, live.data_ptr(), Lx, *tail), "st5_batchnorm_act_bwd_live")
        else:
            hip.check(L.st5_batchnorm_act_fwd(*fwd, *tail), "st5_batchnorm_act_fwd")
            hip.check(L.st5_batchnorm_act_bwd(*bwd, *tail), "st5_batchnorm_act_bwd")
    res = {"existing": [], "live": []}
    for is_live in (False, True):
        for _ in range(5):
            pair(is_live)
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, is_live in (("existing", False), ("live", True)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(group):
                pair(is_live)
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / group)
    return {"rows": rows, "C": C, "group": group, "pair_us": {k: summary(v) for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--commits", default="")
    a = ap.parse_args()
    from speecht5_amd.criterions import SpeechT5Criterion
    from speecht5_amd.update import PretrainUpdate
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arms, lens, chans = {}, None, None
    for name in ARMS:
        args, task, model = build(dev)
        chans = args.postnet_chans
        crit = SpeechT5Criterion(task, use_guided_attn_loss=True, guided_attn_loss_lambda=10.0, guided_attn_loss_sigma=0.4, bce_pos_weight=5.0,
                                 sync_logging=False, device_ntokens=name == "replayed")
        data, lens = batches(dev, task, args, 5, fixed=name != "eager_own")
        Fn.manual_seed(21)
        np.random.seed(8)
        torch.manual_seed(8)
        upd = PretrainUpdate(task, model, crit, data[0], lr=1e-4, clip_norm=25.0, weight_decay=0.1, graph=name == "replayed", micro="in_turn",
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
    wins = sum(r < f for r, f in zip(times["replayed"], times["eager_fixed"]))
    out = {"shape": f"t5_transformer_base bf16, t2s, {B} utterances, fixed shape ({TOKENS}, {FRAMES}), r = {R}, guided attention, dropout 0.15, "
                    "lengths uniform in [half, all] of the shape, in_turn, one micro-batch, stats=True",
           "gpu": torch.cuda.get_device_name(dev), "updates_per_repeat": a.updates, "commits": a.commits, "batches": lens[1:],
           "update_ms": {k: summary(v) for k, v in times.items()},
           "replayed_beats_eager_fixed_in_repeats": f"{wins} of {a.reps}"}
    for upd in arms.values():
        upd.close()
    out["batchnorm_live_vs_existing"] = bn_pairs(dev, chans, max(a.reps, 7))
    txt = json.dumps(out, indent=1)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(txt + "\n")
    print(json.dumps({"update_ms": {k: {m: round(v[m], 3) for m in ("mean", "min", "max")} for k, v in out["update_ms"].items()},
                      "replayed_beats_eager_fixed_in_repeats": out["replayed_beats_eager_fixed_in_repeats"],
                      "bn_pair_us": {k: round(v["median"], 2) for k, v in out["batchnorm_live_vs_existing"]["pair_us"].items()}}))


if __name__ == "__main__":
    main()
