"""Generates tests/golden/tiny_s2t_beam_lm.pt: hypotheses of the VERBATIM reference generator (SpeechT5/speecht5/sequence_generator.py)
decoding the shared tiny model with a shallow-fusion language model (--lm-weight), plus that language model's weights and its
per-layer outputs / logits on a few token batches.

TEST INFRASTRUCTURE ONLY: runs where the reference tree is (imports oracle/ref_stubs.py, oracle/make_golden.py and
oracle/make_golden_beam.py read-only); the tests read only the fixture it writes.

    python tools/make_golden_lm.py

The language model is fairseq's `transformer_lm` (absent from the reference tree) composed from verbatim reference pieces:
  * the layers are the reference's TransformerDecoderLayer(args, no_encoder_attn=True) with decoder_normalize_before=True
    (SpeechT5/speecht5/models/modules/transformer_layer.py, through oracle/ref_stubs.load_reference_models());
  * positions come from the vendored PositionalEmbedding / SinusoidalPositionalEmbedding (SpeechLM/modules.py:414, :1296);
  * only the glue is restated: embed scale sqrt(d), causal mask, final LayerNorm, output projection without bias, log-softmax.
Size: d = 160, 2 heads (head_dim 80), 2 layers, FFN 320, GELU; vocabulary = the text dictionary without <mask> / <ctc_blank>
(V_lm = 34 < V = 36).  Its weights are rounded to bf16 values (stored as bf16, exact in fp32) to keep the fixture small.
The beam-search samples are the ones of tests/golden/tiny_s2t_beam.pt (read from there, not stored again)."""
import math
import os
import sys
from argparse import Namespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_stubs  # noqa: E402
import make_golden as mg  # noqa: E402
import make_golden_beam as mgb  # noqa: E402

LM_SEED = 5
LM_DIMS = dict(decoder_embed_dim=160, decoder_attention_heads=2, decoder_layers=2, decoder_ffn_embed_dim=320, activation_fn="gelu")


class RefLM(nn.Module):
    """fairseq transformer_lm (TransformerLanguageModel + TransformerDecoder, no encoder attention) from reference layers."""

    def __init__(self, layer_cls, vendored, args, vocab, pad):
        super().__init__()
        d = args.decoder_embed_dim
        self.pad = pad
        dec = nn.Module()
        dec.embed_tokens = ref_stubs.Embedding(vocab, d, pad)
        dec.embed_positions = vendored.PositionalEmbedding(1024, d, pad, learned=False)
        dec.layers = nn.ModuleList([layer_cls(args, no_encoder_attn=True) for _ in range(args.decoder_layers)])
        dec.layer_norm = vendored.LayerNorm(d)
        dec.output_projection = nn.Linear(d, vocab, bias=False)
        nn.init.normal_(dec.output_projection.weight, mean=0, std=d ** -0.5)
        dec.register_buffer("version", torch.Tensor([3]))
        self.decoder = dec
        self.embed_scale = math.sqrt(d)

    def forward(self, src_tokens, src_lengths=None):
        dec = self.decoder
        x = self.embed_scale * dec.embed_tokens(src_tokens) + dec.embed_positions(src_tokens)
        x = x.transpose(0, 1)
        pad_mask = src_tokens.eq(self.pad) if src_tokens.eq(self.pad).any() else None
        T = x.shape[0]
        causal = torch.triu(torch.full((T, T), float("-inf")), 1)
        inner = [x]
        for layer in dec.layers:
            x, _, _ = layer(x, None, None, None, self_attn_mask=causal, self_attn_padding_mask=pad_mask)
            inner.append(x)
        x = dec.layer_norm(x).transpose(0, 1)
        return dec.output_projection(x), {"attn": [None], "inner_states": inner}

    def get_normalized_probs(self, net_output, log_probs, sample=None):
        logits = net_output[0].float()
        return F.log_softmax(logits, dim=-1) if log_probs else F.softmax(logits, dim=-1)


class _RowLog:
    """Records the number of hypothesis rows of every LM call (a batch shrink shows as a drop)."""

    def __init__(self, lm):
        self.lm, self.rows = lm, []

    def __call__(self, tokens):
        self.rows.append(int(tokens.shape[0]))
        return self.lm(tokens)

    def get_normalized_probs(self, *a, **k):
        return self.lm.get_normalized_probs(*a, **k)

    def eval(self):
        self.lm.eval()
        return self


def main():
    tiny_model_path = os.path.join(mg.OUT, "tiny_model.pt")
    with open(tiny_model_path, "rb") as f:
        tiny_model_bytes = f.read()          # (shared_model rewrites this committed fixture; it is put back byte for byte)
    ref = ref_stubs.load_reference_models()
    gen_mod = ref_stubs.load_reference_generator()
    args, task, model = mg.shared_model(ref)
    with open(tiny_model_path, "wb") as f:
        f.write(tiny_model_bytes)
    saved = torch.load(tiny_model_path)["state_dict"]
    for k, v in model.state_dict().items():
        if k.endswith("_float_tensor"):
            continue                         # (an uninitialised one-element buffer)
        assert torch.equal(v, saved[k]), f"shared tiny model drifted from tests/golden/tiny_model.pt at {k}"
    d = mgb.FairseqLikeDictionary(30, ["<mask>", "<ctc_blank>"])
    model.eval()
    beam_fx = torch.load(os.path.join(mg.OUT, "tiny_s2t_beam.pt"))
    samples = beam_fx["samples"]

    import importlib
    layer_mod = importlib.import_module("speecht5.models.modules.transformer_layer")
    vendored = ref_stubs.install()
    lm_args = Namespace(**LM_DIMS, dropout=0.1, attention_dropout=0.1, activation_dropout=0.0, decoder_normalize_before=True,
                        quant_noise_pq=0, quant_noise_pq_block_size=8)
    V_lm = len(d) - 2
    torch.manual_seed(LM_SEED)
    lm = RefLM(layer_mod.TransformerDecoderLayer, vendored, lm_args, V_lm, d.pad())
    with torch.no_grad():
        for p in lm.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    lm.eval()

    cases = dict(
        beam1_lm03=dict(sample="two", kw=dict(beam_size=1, max_len_b=12, lm_weight=0.3)),
        beam3_lm03=dict(sample="two", kw=dict(beam_size=3, max_len_b=12, lm_weight=0.3)),
        beam5_lm10=dict(sample="two", kw=dict(beam_size=5, max_len_b=12, lm_weight=1.0)),
        beam3_lm10_minlen=dict(sample="two", kw=dict(beam_size=3, max_len_b=10, min_len=4, lm_weight=1.0)),
        beam2_lm03_prefix=dict(sample="two", kw=dict(beam_size=2, max_len_b=10, lm_weight=0.3), prefix=torch.tensor([[7, 9], [11, 1]])),
        # sentence 0's forced prefix closes it at step 2: it leaves the batch and sentence 1 decodes on alone (rows 2 -> 1).  (Beam 1:
        # a forced prefix gives every other token the same score, and with a wider beam which of those tied candidates -- </s> among
        # them -- lands inside the beam depends on topk's tie order, which differs between devices.)
        beam1_lm03_shrink=dict(sample="two", kw=dict(beam_size=1, max_len_b=12, lm_weight=0.3),
                               prefix=torch.tensor([[7, 9, 2], [11, 1, 1]])),
        beam3_lm03_ctc03=dict(sample="one", kw=dict(beam_size=3, max_len_b=12, ctc_weight=0.3, lm_weight=0.3)),
        beam5_lm03_ctc03=dict(sample="one", kw=dict(beam_size=5, max_len_b=12, ctc_weight=0.3, lm_weight=0.3)),
    )
    out = dict(lm=dict(args=LM_DIMS, vocab=V_lm, pad=d.pad(),
                       state_dict={k: v.to(torch.bfloat16) for k, v in lm.state_dict().items() if k != "decoder.version"}),
               cases={}, batches={})
    for name, c in cases.items():
        log = _RowLog(lm)
        g = gen_mod.SequenceGenerator([model], d, lm_model=log, **c["kw"])
        with torch.no_grad(), mgb._CpuTo():
            hyps = g.generate([model], dict(samples[c["sample"]]), prefix_tokens=c.get("prefix"))
        rec = [[dict(tokens=h["tokens"].clone(), score=float(h["score"]), positional_scores=h["positional_scores"].clone())
                for h in sent] for sent in hyps]
        shrink = any(b < a for a, b in zip(log.rows, log.rows[1:]))
        out["cases"][name] = dict(sample=c["sample"], kw=c["kw"], prefix=c.get("prefix"), hyps=rec, lm_rows=log.rows)
        for si, sent in enumerate(rec):
            gap = sent[0]["score"] - sent[1]["score"] if len(sent) > 1 else float("nan")
            print(f"{name:20s} sent {si}: best {sent[0]['tokens'].tolist()} score {sent[0]['score']:.5f}  "
                  f"(margin to 2nd {gap:.2e}, {len(sent)} hyps){'  [batch shrinks]' if shrink and si == 0 else ''}")

    # per-layer outputs and logits: right-padded rows, and one sequence longer than the initial position table (1024 + pad + 1)
    g = torch.Generator().manual_seed(3)
    padded = torch.randint(4, V_lm, (3, 9), generator=g)
    padded[:, 0] = d.eos()
    padded[1, 6:] = d.pad()
    padded[2, 3:] = d.pad()
    long = torch.randint(4, V_lm, (1, 1100), generator=g)
    long[0, 0] = d.eos()
    keep = slice(1018, 1034)        # (the stored slice of the long sequence: both sides of position 1026)
    with torch.no_grad():
        for name, toks, sl in (("padded", padded, slice(None)), ("long", long, keep)):
            logits, extra = lm(toks)
            out["batches"][name] = dict(tokens=toks, keep=(sl.start, sl.stop), logits=logits[:, sl].clone(),
                                        lprobs=lm.get_normalized_probs((logits,), log_probs=True)[:, sl].clone(),
                                        inner_states=[s.transpose(0, 1)[:, sl].clone() for s in extra["inner_states"]])
    path = os.path.join(ROOT, "tests", "golden", "tiny_s2t_beam_lm.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    np.random.seed(0)
    torch.manual_seed(0)
    main()
