"""Timing of beam search with a shallow-fusion LM (lm_weight 0.3) with the step on the device (SequenceGenerator(decode="device")) and
replayed from a HIP graph (decode="graph") against decode="slots" with the same options (the yardstick: the path these modes did not
cover before, TransformerLanguageModel.decode_step driven from the host).

Base size ASR model (t5_transformer_base, seeded random weights, eval) and a seeded random LM of the transformer_lm_t5 preset (20 layers
x 1280, FFN 6144, 16 heads) over the 83-entry character dictionary of the ASR recipe; seeded clips of 10 s, bf16 by default, (sentences
x beam) in 1 x 1, 1 x 5, 1 x 10, 8 x 1, 8 x 10, each with joint CTC scoring (ctc_weight 0.5, ctc_rows=True) and without.  Everything
else is tools/beam_ctc_timing.py: max_len_b = min_len, the --temperature ladder for the CTC runs (it sharpens the decoder's
distribution so that no hypothesis leaves its CTC candidates; without CTC the first value is used), three arms alternated in one
process after a warm-up call of each, whole generate() calls, host clock around a call that ends in a device synchronise, and the same
fields per shape (plus lm_weight).

    python tools/beam_lm_timing.py [--shapes 1x1 1x5 1x10 8x1 8x10] [--dtype bf16] [--reps 5] [--steps 40] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speecht5_amd import functional as Fn  # noqa: E402
from beam_ctc_timing import ARMS, CTC_WEIGHT, measure  # noqa: E402
from beam_slots_timing import SECONDS, build_model  # noqa: E402
from speech_rows_timing import RATE, batch  # noqa: E402

LM_WEIGHT = 0.3


def build_lm(dev, vocab):
    """A seeded random LM of the transformer_lm_t5 preset (non-trivial LayerNorm affines and biases: every parameter takes part)."""
    from speecht5_amd.transformer_lm import TransformerLanguageModel
    torch.manual_seed(1234)
    lm = TransformerLanguageModel(Namespace(), vocab=vocab, pad=1)
    with torch.no_grad():
        for n, p in lm.named_parameters():
            if n.endswith("layer_norm.weight"):
                p.uniform_(0.5, 1.5)
            elif n.endswith(".bias"):
                p.uniform_(-0.1, 0.1)
    a = lm.args
    assert (a.decoder_layers, a.decoder_embed_dim, a.decoder_ffn_embed_dim, a.decoder_attention_heads) == (20, 1280, 6144, 16)
    return lm.to(dev).eval()


def generator(model, lm, d, arm, beam, steps, temperature, ctc):
    from speecht5_amd.sequence_generator import SequenceGenerator
    return SequenceGenerator([model], d, beam_size=beam, max_len_a=0, max_len_b=steps, min_len=steps, decode=arm, lm_model=lm,
                             lm_weight=LM_WEIGHT, ctc_weight=CTC_WEIGHT if ctc else 0.0, ctc_rows=ctc, temperature=temperature)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1x1", "1x5", "1x10", "8x1", "8x10"], help="sentences x beam")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--temperature", type=float, nargs="+", default=[0.25, 0.05])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    results, failed = [], []
    dtype = torch.float32 if a.dtype == "fp32" else torch.bfloat16
    model, d = build_model(dev, dtype)
    assert len(d) == 83
    lm = build_lm(dev, len(d))
    med = statistics.median
    with torch.no_grad():
        for shape in a.shapes:
            bsz, beam = (int(v) for v in shape.split("x"))
            wav, pad = batch([SECONDS * RATE] * bsz, dev, seed=7)
            sample = {"net_input": {"source": wav, "padding_mask": pad}}
            for ctc in (True, False):
                r = dict(dtype=a.dtype, bsz=bsz, beam=beam, steps=a.steps + 1, lm_weight=LM_WEIGHT, ctc_weight=CTC_WEIGHT if ctc else 0.0,
                         ctc_rows=ctc, temperature=None, key_error_at_temperature=[])
                for temperature in (a.temperature if ctc else a.temperature[:1]):
                    gens = {arm: generator(model, lm, d, arm, beam, a.steps, temperature, ctc) for arm in ARMS}
                    try:
                        outs, times = measure(gens, sample, a.reps)
                    except KeyError:
                        torch.cuda.synchronize()
                        r["key_error_at_temperature"].append(temperature)
                        continue
                    sl, de, gr = times["slots"], times["device"], times["graph"]
                    same = {arm: sum(outs["slots"][b][0]["tokens"].tolist() == outs[arm][b][0]["tokens"].tolist() for b in range(bsz))
                            for arm in ("device", "graph")}
                    g = gens["graph"]
                    r.update(temperature=temperature, slots_ms=[round(t * 1e3, 1) for t in sl], device_ms=[round(t * 1e3, 1) for t in de],
                             graph_ms=[round(t * 1e3, 1) for t in gr], slots_spread_ms=round((max(sl) - min(sl)) * 1e3, 1),
                             slots_over_device=round(med(sl) / med(de), 3), slots_over_graph=round(med(sl) / med(gr), 3),
                             every_graph_repeat_beats_every_slots_repeat=max(gr) < min(sl),
                             graph_polls=g.beam_polls, graph_replays=g.beam_graph_replays,
                             same_best_hypothesis_as_slots={k: f"{v} of {bsz}" for k, v in same.items()})
                    break
                results.append(r)
                print(json.dumps(r), flush=True)
                if r["temperature"] is None:
                    failed.append(f"{shape} ctc")
                    print(f"beam_lm_timing: {shape} with CTC NOT MEASURED: every arm set raised the CTC KeyError at temperatures "
                          f"{a.temperature}", file=sys.stderr, flush=True)
                if a.json:
                    with open(a.json, "w") as f:
                        json.dump(results, f, indent=1)
                del gens
                torch.cuda.empty_cache()
    Fn.set_compute_dtype(torch.float32)
    if failed:
        sys.exit(f"beam_lm_timing: no timing for {failed}; pass a sharper --temperature")


if __name__ == "__main__":
    main()
