"""Cost of the validation UER / WER counts (speecht5_amd/asr_metrics.py, csrc/asr_metrics.hip) in an ASR fine-tuning valid_step.

Base size (t5_transformer_base, seeded random weights), fp32, an 83-entry character dictionary with a word separator (`|`,
post_process "letter"), seeded clips of 10 s (499 encoder frames), targets of 150-200 units with a separator every 4-8 units,
ce_weight = ctc_weight = 0.5, B in {8, 32}.

valid  whole `task.valid_step` calls, host clock around a call that ends in a device synchronise, three arms ALTERNATED in one
       process after a warm-up call of each, every repeat kept:
         parent       the criterion module of the parent commit (no counts), given as a file:  git show HEAD~1:speecht5_amd/criterions.py
         sync         this commit, sync_logging=True (Python numbers: the step's .item() reads)
         device       this commit, sync_logging=False (device scalars)
       The model, the library and the sample are shared, so the arms differ in the criterion code alone.  A random model's greedy
       decoding is short (its length is recorded); `--posterior` replaces the CTC posterior the criterion sees by a made one:
         trained      the target's units with about 8 % of them replaced, each held for two frames between blanks
         worst        a different unit in every frame: the prediction is as long as T, the edit distance walks T + L diagonals
kernels  the four entry points alone at the same shapes, HIP events around groups of launches.
count    two valid_step calls of this commit (sync_logging=False) in a fresh process, for a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/asr_metrics_timing.py --mode count --bsz 8

    python tools/asr_metrics_timing.py --mode valid --parent-criterions FILE [--bsz 8 32] [--reps 7] [--json out.json]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time
from argparse import Namespace
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import asr_metrics as A  # noqa: E402
from speecht5_amd import functional as Fn  # noqa: E402
from speech_rows_timing import RATE, batch  # noqa: E402

SECONDS = 10
SYMBOLS = ["|", "'"] + [chr(c) for c in range(ord("a"), ord("z") + 1)] + [f"x{i}" for i in range(49)]     # 77 symbols -> 83 entries


def build(dev):
    from speecht5_amd.speecht5 import t5_transformer_base
    from speecht5_amd.task import SpeechT5Task, _Dictionary
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()
    args = Namespace(label_rates=50, sample_rate=RATE, speech_odim=80, bert_init=True, use_codebook=False, share_input_output_embed=True,
                     encoder_layerdrop=0.0, decoder_layerdrop=0.0, t5_task="s2t")
    t5_transformer_base(args)
    task = SpeechT5Task(args, {"text": _Dictionary(SYMBOLS)})
    torch.manual_seed(4246)
    return task, task.build_model(args).to(dev)


def make_sample(task, B, dev, seed=5):
    d = task.target_dictionary
    g = torch.Generator().manual_seed(seed + B)
    wav, pad = batch([SECONDS * RATE] * B, dev, seed=seed)
    lens = torch.randint(150, 201, (B,), generator=g)
    L = int(lens.max()) + 1
    target = torch.full((B, L), d.pad(), dtype=torch.long)
    for b in range(B):
        n = int(lens[b])
        row = torch.randint(d.index("a"), d.index("z") + 1, (n,), generator=g)
        p = int(torch.randint(4, 9, (1,), generator=g))
        while p < n:
            row[p] = d.index("|")
            p += int(torch.randint(4, 9, (1,), generator=g))
        target[b, :n] = row
        target[b, n] = d.eos()
    prev = torch.cat([torch.full((B, 1), d.eos(), dtype=torch.long), target[:, :-1]], 1).masked_fill(target == d.pad(), d.pad())
    prev[prev == d.eos()] = d.pad()
    prev[:, 0] = d.eos()
    return dict(net_input=dict(source=wav, padding_mask=pad, prev_output_tokens=prev.to(dev), task_name="s2t"), target=target.to(dev),
                target_lengths=(lens + 1).to(dev), ntokens=int(lens.sum()) + B, task_name="s2t", id=torch.arange(B))


def made_posterior(kind, target, T, V, blank, d, seed=9):
    """[T, B, V] log-probabilities on the host whose greedy decoding is `kind` (see the module docstring)."""
    g = torch.Generator().manual_seed(seed)
    B = target.size(0)
    path = torch.full((B, T), blank, dtype=torch.long)
    lo, hi = d.index("a"), d.index("z")
    for b in range(B):
        if kind == "worst":
            path[b] = lo + (torch.arange(T) % 2)
            continue
        units = [int(x) for x in target[b].tolist() if x not in (d.pad(), d.eos())]
        t = 0
        for u in units:
            if t + 3 > T:
                break
            if float(torch.rand(1, generator=g)) < 0.08:
                u = int(torch.randint(lo, hi + 1, (1,), generator=g))
            path[b, t] = path[b, t + 1] = u
            t += 3 if t % 2 else 2
    logits = torch.randn(T, B, V, generator=g)
    logits.scatter_add_(2, path.t().unsqueeze(-1), torch.full((T, B, 1), 8.0))
    return torch.log_softmax(logits, -1)


def load_parent(path):
    spec = importlib.util.spec_from_file_location("speecht5_amd._parent_criterions", path)
    mod = importlib.util.module_from_spec(spec)
    mod.__package__ = "speecht5_amd"
    import speecht5_amd.fairseq_compat as fc
    registry = getattr(fc, "CRITERION_REGISTRY", None)       # the in-tree registry refuses a second `speecht5`: restore it afterwards
    saved = dict(registry) if isinstance(registry, dict) else None
    if saved is not None:
        registry.clear()
    try:
        spec.loader.exec_module(mod)
    finally:
        if saved is not None:
            registry.clear()
            registry.update(saved)
    return mod


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def criterion(module, task, sync):
    cfg = SimpleNamespace(zero_infinity=True, post_process="letter")
    return module.SpeechT5Criterion(task, sentence_avg=False, ce_weight=0.5, ctc_weight=0.5, report_accuracy=True, cfg=cfg, sync_logging=sync)


def with_posterior(model, lp):
    """The model's CTC posterior replaced by lp (device); returns the undo."""
    inner = model.get_normalized_probs_for_ctc
    model.get_normalized_probs_for_ctc = lambda net_output, log_probs=True: lp
    return lambda: setattr(model, "get_normalized_probs_for_ctc", inner)


def valid_mode(args, dev, results):
    from speecht5_amd import criterions as this
    task, model = build(dev)
    parent = load_parent(args.parent_criterions) if args.parent_criterions else None
    d = task.target_dictionary
    blank = d.index("<ctc_blank>")
    for B in args.bsz:
        sample = make_sample(task, B, dev)
        for kind in args.posterior:
            arms = {"sync": criterion(this, task, True), "device": criterion(this, task, False)}
            if parent is not None:
                arms = dict(parent=criterion(parent, task, True), **arms)
            undo = None
            if kind != "model":
                with torch.no_grad():
                    model.eval()
                    T = model(**sample["net_input"])[1]["encoder_out"][0].size(0)
                undo = with_posterior(model, made_posterior(kind, sample["target"].cpu(), T, len(d), blank, d).to(dev))
            try:
                logs = {}
                for name, c in arms.items():                       # warm-up of every arm
                    logs[name] = task.valid_step(sample, model, c)[2]
                sec = {name: [] for name in arms}
                for _ in range(args.reps):
                    for name, c in arms.items():
                        sec[name].append(timed(lambda: task.valid_step(sample, model, c))[0])
            finally:
                if undo is not None:
                    undo()
            counts = {k: int(logs["device"][k]) for k in A.KEYS}
            assert counts == {k: logs["sync"][k] for k in A.KEYS}
            with torch.no_grad():
                lp, n = arms["sync"].text_criterion._ctc_inputs(model, model(**sample["net_input"])[1]) if kind == "model" else (None, None)
            med = {name: statistics.median(v) for name, v in sec.items()}
            res = dict(mode="valid", B=B, posterior=kind, frames=499, counts=counts,
                       ms={name: [round(v * 1e3, 3) for v in vs] for name, vs in sec.items()},
                       median_ms={name: round(v * 1e3, 3) for name, v in med.items()})
            if lp is not None:
                res["greedy_units_per_sentence"] = Fn.ctc_greedy_rows(lp, n, blank)[1].tolist()
            if parent is not None:
                res["added_ms_sync_minus_parent"] = round((med["sync"] - med["parent"]) * 1e3, 3)
                res["added_ms_device_minus_parent"] = round((med["device"] - med["parent"]) * 1e3, 3)
                res["parent_spread_ms"] = round((max(sec["parent"]) - min(sec["parent"])) * 1e3, 3)
                assert all(logs["parent"][k] == logs["sync"][k] for k in ("loss", "ctc_loss", "ce_loss", "n_correct")), "the arms disagree"
            results.append(res)
            print(json.dumps(res), flush=True)


def events_us(fn, groups=7, per_group=20):
    for _ in range(5):
        fn()
    out = []
    for _ in range(groups):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_group):
            fn()
        e1.record()
        e1.synchronize()
        out.append(round(e0.elapsed_time(e1) / per_group * 1e3, 2))
    return out


def kernels_mode(args, dev, results):
    task, _ = build(torch.device("cpu"))
    d = task.target_dictionary
    blank, V, T = d.index("<ctc_blank>"), len(d), 499
    tab = A.byte_table(d, "letter", dev)   # (no cache: built once here)
    tables = {}
    for B in args.bsz:
        target = make_sample(task, B, torch.device("cpu"))["target"]
        tgt, tgt_len = A.strip_pad_eos(target.to(dev), d.pad(), d.eos())
        in_len = torch.full((B,), T, dtype=torch.long, device=dev)
        for kind in ("trained", "worst"):
            lp = made_posterior(kind, target, T, V, blank, d).to(dev)
            pred, pred_len = Fn.ctc_greedy_rows(lp, in_len, blank)
            pw = Fn.tokens_to_words(pred, pred_len, tab.offsets, tab.data, tab.max_symbol_bytes)
            tw = Fn.tokens_to_words(tgt, tgt_len, tab.offsets, tab.data, tab.max_symbol_bytes)
            p_ids, t_ids = Fn.word_ids(pw, tw)
            p_ids, t_ids = p_ids[:, :T].contiguous(), t_ids[:, :tgt.size(1)].contiguous()
            us = dict(
                ctc_greedy_rows=events_us(lambda: Fn.ctc_greedy_rows(lp, in_len, blank)),
                edit_distance_units=events_us(lambda: Fn.edit_distance_rows(pred, pred_len, tgt, tgt_len)),
                tokens_to_words_pred=events_us(lambda: Fn.tokens_to_words(pred, pred_len, tab.offsets, tab.data, tab.max_symbol_bytes, pw.err)),
                tokens_to_words_target=events_us(lambda: Fn.tokens_to_words(tgt, tgt_len, tab.offsets, tab.data, tab.max_symbol_bytes, tw.err)),
                word_ids=events_us(lambda: Fn.word_ids(pw, tw)),
                edit_distance_words=events_us(lambda: Fn.edit_distance_rows(p_ids, pw.n, t_ids, tw.n)),
                all_of_count_errors=events_us(lambda: A.count_errors(lp, in_len, target.to(dev), d, blank, "letter", tables)))
            res = dict(mode="kernels", B=B, posterior=kind, T=T, V=V, units_pred=[int(pred_len.min()), int(pred_len.max())],
                       units_target=[int(tgt_len.min()), int(tgt_len.max())], words_pred=[int(pw.n.min()), int(pw.n.max())],
                       words_target=[int(tw.n.min()), int(tw.n.max())], us_median={k: statistics.median(v) for k, v in us.items()}, us_all=us,
                       note="launches back to back on one stream, wrapper allocations and launch overhead included")
            results.append(res)
            print(json.dumps(res), flush=True)


def count_mode(args, dev):
    from speecht5_amd import criterions as this
    task, model = build(dev)
    sample = make_sample(task, args.bsz[0], dev)
    c = criterion(this, task, False)
    for _ in range(2):
        log = task.valid_step(sample, model, c)[2]
    torch.cuda.synchronize()
    print({k: int(log[k]) for k in A.KEYS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["valid", "kernels", "count"], default="valid")
    ap.add_argument("--bsz", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--posterior", nargs="+", default=["model", "trained", "worst"], choices=["model", "trained", "worst"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-criterions", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []
    if args.mode == "valid":
        valid_mode(args, dev, results)
    elif args.mode == "kernels":
        kernels_mode(args, dev, results)
    else:
        count_mode(args, dev)
    if args.json:
        old = json.load(open(args.json)) if os.path.exists(args.json) else []
        json.dump(old + results, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
