"""Measures the figures the bars of tests/test_s2s_gpu.py refer to and writes them to profiles/s2s_parity.txt (needs a GPU):

    python tools/s2s_parity.py [--out profiles/s2s_parity.txt]

  * se_predict kernels: max abs error against the fp64 restatement, forward and backward, for torch's own fp32 evaluation on the
    device and for the kernels, per shape and mode (the test allows twice torch's figure);
  * tiny whole-model cases against the verbatim reference's fixture: the largest error of every kind of quantity, relative to the
    tolerance the test applies to it;
  * ragged log-mel: LogMelFilterBank.rows against the oracle and against the per-item __call__."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import logmel_oracle as O  # noqa: E402
from tests import test_s2s_gpu as T  # noqa: E402
from tests.util import G  # noqa: E402


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2s_parity.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"s2s parity figures ({torch.cuda.get_device_name(0)}); tools/s2s_parity.py", ""]
    lines.append("se_predict kernels: max abs error against fp64 (torch fp32 on the device | kernels); the test allows 2 x torch")
    for mode in ("masking", "delta"):
        for shape in T.SE_SHAPES:
            e, _, _ = T.se_errors(dev, shape, mode)
            lines.append(f"  {mode:8s} {str(shape):12s} forward {e['torch_fwd']:.3e} | {e['ours_fwd']:.3e}   backward {e['torch_bwd']:.3e} | {e['ours_bwd']:.3e}")
    lines += ["", "tiny model cases against tests/golden/tiny_s2s.pt: largest error relative to the reference tensor's scale (test tolerance)"]
    fx = torch.load(os.path.join(G, "tiny_s2s.pt"), weights_only=False)
    for name in T.CASES:
        case = fx["cases"][name]
        model, sample, out, loss, ss, log, got = T.case_errors(fx, name, dev)
        outs = max(rel(g, case["train"][k]) for g, k in zip(out[:3], ("before", "after", "stop_logits")))
        attn = max(rel(x, y) for x, y in zip(out[3], case["train"]["attn"]))
        logs = max(abs(log[k] - v) / max(abs(v), 1.0) for k, v in case["log"].items())
        scale = max(case["grads"]["norms"].values())
        norms = max((abs((float(got[n].double().norm()) if n in got else 0.0) - r) - 1e-4 * scale) / max(r, 1e-30) for n, r in case["grads"]["norms"].items())
        full = max(float((got[n].double().cpu() - r.double()).abs().max()) / (2e-3 * max(float(r.abs().max()), 1e-6) + 1e-4 * scale)
                   for n, r in case["grads"]["full"].items())
        lines.append(f"  {name:11s} outputs {outs:.2e} (2e-4)  attn {attn:.2e} (2e-4)  loss {rel(loss, case['loss']):.2e} (2e-4)  log {logs:.2e} (3e-4)  "
                     f"grad norms beyond the floor {max(norms, 0.0):.2e} (2e-3)  full grads, fraction of their bar {full:.2f}")
    for name in ("recipe", "masking"):
        case = fx["cases"][name]
        model = T.build_case(fx, name, dev)
        model.eval()
        wav = fx["gen_clip"].to(dev)
        spk = fx["samples"][case["case"]["r"]]["net_input"]["spkembs"][:1].to(dev)
        mel, probs, _ = model.generate_speech(source=wav, padding_mask=torch.zeros(wav.shape, dtype=torch.bool, device=dev), spkembs=spk)
        lines.append(f"  {name:11s} generate_speech(source): mel {rel(mel, case['generated_mel']):.2e} (1e-3)  probs {rel(probs, case['generated_probs']):.2e} (1e-3)")
    lines += ["", "ragged log-mel (LogMelFilterBank.rows, one call over all lengths): max abs difference to the oracle (bar 2e-3) and to __call__ per item"]
    fb, wavs, rows, single = T.rows_case(dev)
    for w, got, one in zip(wavs, rows, single):
        lines.append(f"  {len(w):5d} samples, {got.shape[0]:2d} frames: oracle {np.abs(got.numpy() - O.logmelfilterbank(w.numpy())).max():.3e}   "
                     f"__call__ {float((got - one).abs().max()):.3e}   bit-equal {bool(torch.equal(got, one))}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
