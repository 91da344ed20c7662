"""The library entry points (st5_*) of one whole decode call in "device" mode, name by name and in order, for the device-stepped TTS
decode (generate_speech_batch) and the device-stepped ASR beam search (SequenceGenerator) on the tiny golden models.  A refactor of
the step's host code must leave every list as it is: tests/test_step_program_gpu.py compares them with
tests/golden/decode_step_calls.json, which this tool wrote on the tree BEFORE such a change.

    python tools/decode_step_calls.py --out tests/golden/decode_step_calls.json

Every case makes one call untraced first (it fills the weight caches), then the traced one.  TTS: threshold=2.0, which no stop
probability reaches and which also stands for both length ratios, so the call runs to a cap of 2 T / r steps, past one poll."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TTS_MODELS = {"pre-ln spk": (True, True), "pre-ln no-spk": (True, False), "post-ln spk": (False, True)}      # (pre_ln, speaker embeddings)
ASR_CASES = {"plain": (False, False), "ctc": (True, False), "lm": (False, True), "ctc lm": (True, True)}      # (CTC, LM)
ASR_KW = dict(beam_size=3, max_len_b=9, decode="device")


def record(dev):
    """{case: [entry point names]} of every case."""
    from speecht5_amd import functional as Fn
    from speecht5_amd.sequence_generator import SequenceGenerator
    from tests.test_beam_lm_device_gpu import _tiny_lm
    from tests.test_ctc_rows_gpu import _count_lib_calls
    from tests.test_tts_graph_gpu import _tiny
    from tests.util import Task, build_tiny, load_golden, to_dev
    out = {}
    try:
        _, fx = load_golden("tiny_t2s.pt")
        ni = fx["sample"]["net_input"]
        toks, spk = ni["src_tokens"].to(dev), ni["spkembs"].to(dev)
        for name, (pre_ln, with_spk) in TTS_MODELS.items():
            model, _ = _tiny(dev, torch.float32, pre_ln)
            for need_attn in (False, True):
                def call():
                    Fn.manual_seed(1234)
                    with torch.no_grad():
                        return model.generate_speech_batch(src_tokens=toks, spkembs=spk if with_spk else None, need_attn=need_attn,
                                                           decode="device", threshold=2.0)
                call()
                _, out[f"tts {name} need_attn={need_attn}"] = _count_lib_calls(call)
            Fn.weight_cache.clear()
        _, fx = load_golden("tiny_s2t_beam.pt")
        _, fx_lm = load_golden("tiny_s2t_beam_lm.pt")
        model, _ = build_tiny(dev, torch.float32)
        model.eval()
        d, lm = Task().dicts["text"], _tiny_lm(fx_lm, dev)
        sample = to_dev(fx["samples"]["one"], dev)
        for name, (ctc, with_lm) in ASR_CASES.items():
            kw = dict(ASR_KW, **(dict(ctc_weight=0.3, ctc_rows=True) if ctc else {}), **(dict(lm_model=lm, lm_weight=0.3) if with_lm else {}))

            def call():
                return SequenceGenerator([model], d, **kw).generate([model], sample)
            call()
            _, out[f"asr {name}"] = _count_lib_calls(call)
    finally:
        Fn.set_compute_dtype(torch.float32)
        Fn.weight_cache.clear()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    calls = record(torch.device("cuda:0"))
    torch.cuda.synchronize()
    with open(a.out, "w") as f:
        json.dump(calls, f, indent=0)
        f.write("\n")
    for name, log in calls.items():
        print(f"{name}: {len(log)} calls")


if __name__ == "__main__":
    main()
