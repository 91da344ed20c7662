"""Seeded dump of generate_speech_batch and synthesize_batch with `decode` left at its default, for a byte comparison between two
trees (the default path must keep its bits): prints one SHA-256 per (dtype, entry point) over every returned tensor.

    python tools/tts_graph_dump.py > dump.txt        # run on both trees, then diff the two files
    python tools/tts_graph_dump.py --decode device graph > dump.txt      # the same for the device-stepped modes

Tiny golden model and tiny golden vocoder, text rows and speech rows, pre-net dropout 0.5 under Fn.manual_seed, fp32 and bf16."""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speecht5_amd import functional as Fn  # noqa: E402


def digest(outs):
    h = hashlib.sha256()
    for row in outs:
        for t in row:
            if t is not None:
                h.update(t.detach().float().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--decode", nargs="+", default=["eager"], choices=["eager", "device", "graph"])
    for mode in ap.parse_args().decode:
        dump({} if mode == "eager" else {"decode": mode}, "" if mode == "eager" else f"decode={mode} ")


def dump(kw, tag):
    from speecht5_amd.hifigan import SpeechT5HifiGan
    from tests.util import build_tiny, load_golden
    dev = torch.device("cuda:0")
    _, fx = load_golden("tiny_t2s.pt")
    ni = fx["sample"]["net_input"]
    toks, spk = ni["src_tokens"].to(dev), ni["spkembs"].to(dev)
    g = torch.Generator().manual_seed(55)
    n = [16000, 40000, 27200]
    src = torch.zeros(3, max(n))
    pad = torch.ones(3, max(n), dtype=torch.bool)
    for b, m in enumerate(n):
        src[b, :m] = torch.randn(m, generator=g) * 0.1
        pad[b, :m] = False
    src, pad = src.to(dev), pad.to(dev)
    hf = torch.load(os.path.join(ROOT, "tests", "golden", "tiny_hifigan.pt"), weights_only=False)
    for dname, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        model, _ = build_tiny(dev, dtype)
        model.eval()
        voc = None
        if dtype == torch.float32:
            voc = SpeechT5HifiGan(**hf["config"]).eval()
            voc.load_state_dict(hf["state_dict"])
            voc = voc.to(dev)
        tac = model.speech_decoder_prenet.decoder_prenet[0][0]
        with torch.no_grad():
            for p in (0.0, 0.5):
                tac.dropout_rate = p
                Fn.manual_seed(1234)
                print(tag + dname, f"dropout={p}", "generate_speech_batch text  ",
                      digest(model.generate_speech_batch(src_tokens=toks, spkembs=spk, **kw)))
                print(tag + dname, f"dropout={p}", "generate_speech_batch speech",
                      digest(model.generate_speech_batch(source=src, padding_mask=pad, spkembs=spk, **kw)))
                print(tag + dname, f"dropout={p}", "synthesize_batch            ",
                      digest(model.synthesize_batch(src_tokens=toks, spkembs=spk, vocoder=voc, need_attn=True, **kw)),
                      "vocoder" if voc else "no vocoder")
        Fn.weight_cache.clear()
    Fn.set_compute_dtype(torch.float32)


if __name__ == "__main__":
    main()
