"""Dump of the device-stepped ASR beam search for a byte comparison between two trees: one SHA-256 per (dtype, case, mode) over the
tokens, the score and the positional scores of every hypothesis, on the tiny golden model (tests/golden/tiny_s2t_beam.pt, its
two-sentence sample for the cases without CTC, the one-sentence sample with) -- plain, with ctc_weight 0.3 / ctc_rows, with the tiny LM
(lm_weight 0.3), and with both; decode="device" and "graph"; fp32 and bf16.

    python tools/beam_graph_dump.py > dump.txt        # run on both trees, then diff the two files"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speecht5_amd import functional as Fn  # noqa: E402

CASES = {"plain": (False, False), "ctc": (True, False), "lm": (False, True), "ctc lm": (True, True)}      # (CTC, LM)


def digest(out):
    h = hashlib.sha256()
    for hyps in out:
        h.update(len(hyps).to_bytes(4, "little"))
        for hyp in hyps:
            for k in ("tokens", "score", "positional_scores"):
                h.update(hyp[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    from speecht5_amd.sequence_generator import SequenceGenerator
    from tests.test_beam_lm_device_gpu import _tiny_lm
    from tests.util import Task, build_tiny, load_golden, to_dev
    dev = torch.device("cuda:0")
    _, fx = load_golden("tiny_s2t_beam.pt")
    _, fx_lm = load_golden("tiny_s2t_beam_lm.pt")
    d = Task().dicts["text"]
    for dname, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        model, _ = build_tiny(dev, dtype)
        model.eval()
        lm = _tiny_lm(fx_lm, dev)
        for name, (ctc, with_lm) in CASES.items():
            kw = dict(beam_size=3, max_len_b=12, **(dict(ctc_weight=0.3, ctc_rows=True) if ctc else {}),
                      **(dict(lm_model=lm, lm_weight=0.3) if with_lm else {}))
            sample = to_dev(fx["samples"]["one" if ctc else "two"], dev)
            for mode in ("device", "graph"):
                gen = SequenceGenerator([model], d, decode=mode, **kw)
                out = gen.generate([model], sample)
                torch.cuda.synchronize()
                print(dname, f"{name:7s}", f"{mode:6s}", digest(out), f"steps={gen.beam_device_steps + gen.beam_graph_replays} polls={gen.beam_polls}")
        Fn.weight_cache.clear()
    Fn.set_compute_dtype(torch.float32)


if __name__ == "__main__":
    main()
