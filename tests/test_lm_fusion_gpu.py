"""Shallow-fusion language model on the HIP kernels (speecht5_amd/transformer_lm.py, csrc/lm_decode.hip) and its use in ASR beam search
(speecht5_amd/sequence_generator.py with lm_model=...).

1. hypotheses of the VERBATIM reference generator with the reference-composed LM (tests/golden/tiny_s2t_beam_lm.pt, written by
   tools/make_golden_lm.py): token ids of every hypothesis bit-exact and in order, scores within SCORE_TOL;
2. st5_lm_decode_attn alone against an fp64 gather over random ancestry tables (unreferenced slots hold NaN);
3. the incremental decode path = the full-prefix forward under random beam reorders and a batch shrink (tiny and real size);
4. forward() against tests/lm_reference.py (real size; tiny size with T > 1024);
5. st5_lm_fuse_logprobs; 6. bf16 compute mode; 7. state-dict layout and build_generator's conversion of a fairseq-layout LM."""
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.lm_reference import lm_forward
from tests.test_generator_gpu import SCORE_TOL
from tests.util import Task, build_tiny, load_golden, to_dev

pytestmark = pytest.mark.gpu

REAL = dict(decoder_embed_dim=1280, decoder_attention_heads=16, decoder_layers=20, decoder_ffn_embed_dim=6144, activation_fn="gelu")


@pytest.fixture(scope="module")
def fx():
    return load_golden("tiny_s2t_beam_lm.pt")[1]


def _tiny_lm(fx, dev):
    from speecht5_amd.transformer_lm import TransformerLanguageModel
    sd = {k: v.float() for k, v in fx["lm"]["state_dict"].items()}
    lm = TransformerLanguageModel.from_state_dict(sd, Namespace(**fx["lm"]["args"]), pad=fx["lm"]["pad"])
    return lm.to(dev).eval()


@pytest.fixture(scope="module")
def real_lm(cuda):
    from speecht5_amd import functional as Fn
    from speecht5_amd.transformer_lm import TransformerLanguageModel
    Fn.set_compute_dtype(torch.float32)
    torch.manual_seed(1234)
    lm = TransformerLanguageModel(Namespace(**REAL), vocab=83, pad=1)
    with torch.no_grad():                 # (non-trivial LayerNorm affines and biases: every parameter takes part)
        for n, p in lm.named_parameters():
            if n.endswith("layer_norm.weight"):
                p.uniform_(0.5, 1.5)
            elif n.endswith(".bias"):
                p.uniform_(-0.1, 0.1)
    yield lm.to(cuda).eval()
    Fn.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. hypotheses vs the verbatim reference generator
# ------------------------------------------------------------------------------------------------------------------------------
CASES = ["beam1_lm03", "beam3_lm03", "beam5_lm10", "beam3_lm10_minlen", "beam2_lm03_prefix", "beam1_lm03_shrink", "beam3_lm03_ctc03",
         "beam5_lm03_ctc03"]


@pytest.fixture(scope="module")
def gen_setup(cuda, fx):
    from speecht5_amd import functional as Fn
    model, _ = build_tiny(cuda, torch.float32)
    model.eval()
    yield model, _tiny_lm(fx, cuda), Task().dicts["text"]
    Fn.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("name", CASES)
def test_lm_fused_hypotheses_equal_reference_generator(cuda, fx, gen_setup, name):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, lm, d = gen_setup
    case = fx["cases"][name]
    calls = []
    step = lm.decode_step

    def counted(*a, **k):
        calls.append(1)
        return step(*a, **k)

    lm.decode_step = counted
    try:
        gen = SequenceGenerator([model], d, lm_model=lm, **case["kw"])
        sample = to_dev(fx_samples()[case["sample"]], cuda)
        prefix = case["prefix"].to(cuda) if case["prefix"] is not None else None
        hyps = gen.generate([model], sample, prefix_tokens=prefix)
    finally:
        del lm.decode_step
    assert len(calls) == len(case["lm_rows"]), "the HIP LM must run one incremental step per beam-search step"
    assert len(hyps) == len(case["hyps"])
    for si, (got, ref) in enumerate(zip(hyps, case["hyps"])):
        assert len(got) == len(ref), f"sentence {si}: {len(got)} hypotheses, reference {len(ref)}"
        for hi, (g, r) in enumerate(zip(got, ref)):
            assert g["tokens"].cpu().tolist() == r["tokens"].tolist(), f"sentence {si} hypothesis {hi}"
            assert abs(float(g["score"]) - r["score"]) <= SCORE_TOL * max(1.0, abs(r["score"])), (si, hi, float(g["score"]), r["score"])
            np.testing.assert_allclose(g["positional_scores"].cpu().numpy(), r["positional_scores"].numpy(), atol=2e-3, rtol=0)


_SAMPLES = {}


def fx_samples():
    if not _SAMPLES:
        _SAMPLES.update(load_golden("tiny_s2t_beam.pt")[1]["samples"])
    return _SAMPLES


# ------------------------------------------------------------------------------------------------------------------------------
# 2. st5_lm_decode_attn against an fp64 gather
# ------------------------------------------------------------------------------------------------------------------------------
def _attn_case(dev, rows, t, H, hd, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    C = H * hd
    rows_cap, Tmax = rows + 3, t + 2
    anc = torch.randint(0, rows_cap, (rows, Tmax), generator=g, device=dev, dtype=torch.int32)
    shared = torch.rand(rows, Tmax, generator=g, device=dev) < 0.5      # half the entries from a few shared parents
    anc = torch.where(shared, torch.randint(0, 2, (rows, Tmax), generator=g, device=dev, dtype=torch.int32), anc)
    anc[:, t:] = -7                                                      # (never read: positions >= t)
    kv = torch.full((rows_cap, Tmax, 2 * C), float("nan"), device=dev)
    used = torch.zeros(rows_cap, Tmax, dtype=torch.bool, device=dev)
    used[anc[:, :t].long(), torch.arange(t, device=dev).unsqueeze(0).expand(rows, t)] = True
    kv[used] = torch.randn(int(used.sum()), 2 * C, generator=g, device=dev) * 1.5
    q = torch.randn(rows, C, generator=g, device=dev) * 1.5
    return q.to(dtype), kv.to(dtype), anc                                # (the reference sees the rounded inputs)


def _attn_ref(q, kv, anc, t, H, hd, dtype=torch.float64):
    rows, C = q.shape
    j = torch.arange(t, device=q.device)
    rowsel = kv[anc[:, :t].long(), j.unsqueeze(0)].to(dtype)             # [rows, t, 2C]
    k = rowsel[..., :C].view(rows, t, H, hd).transpose(1, 2)
    v = rowsel[..., C:].view(rows, t, H, hd).transpose(1, 2)
    qq = q.to(dtype).view(rows, H, 1, hd)
    p = torch.softmax((qq @ k.transpose(-1, -2)) * hd ** -0.5, dim=-1)
    return (p @ v).view(rows, C)


@pytest.mark.parametrize("t", [1, 2, 63, 64, 65, 1000])
@pytest.mark.parametrize("rows", [1, 5, 40, 80])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hd,H", [(80, 16), (64, 12)])
def test_decode_attn_matches_fp64_gather(cuda, hd, H, dtype, rows, t):
    from speecht5_amd import functional as Fn
    q, kv, anc = _attn_case(cuda, rows, t, H, hd, dtype, seed=rows * 7919 + t)
    out = Fn.lm_decode_attn(q, kv, anc, t, H, hd)
    torch.cuda.synchronize()
    ref = _attn_ref(q, kv, anc, t, H, hd)
    got = out.double()
    assert torch.isfinite(got).all(), "an unreferenced (NaN) slot reached the output"
    if dtype == torch.float32:
        e32 = (_attn_ref(q, kv, anc, t, H, hd, torch.float32).double() - ref).abs().max().item()
        err = (got - ref).abs().max().item()
        assert err <= 4 * e32 + 1e-7, (err, e32)
    else:
        err = ((got - ref).abs() - (2 ** -7 * ref.abs() + 2e-3)).max().item()
        assert err <= 0, err


def test_decode_attn_refuses_other_head_dims(cuda):
    from speecht5_amd import hip
    q = torch.zeros(2, 4 * 96, device=cuda)
    kv = torch.zeros(2, 4, 2 * 4 * 96, device=cuda)
    anc = torch.zeros(2, 4, dtype=torch.int32, device=cuda)
    for hd in (32, 96, 128):
        rc = hip.lib().st5_lm_decode_attn(q.data_ptr(), q.shape[1], kv.data_ptr(), 2, 4, anc.data_ptr(), 4, 2, 3, 4, hd, q.data_ptr(),
                                          q.shape[1], 0, hip.F32, hip.stream())
        assert rc == 1, (hd, rc)


def test_decode_attn_broken_ancestry_gives_nan(cuda):
    from speecht5_amd import functional as Fn
    q, kv, anc = _attn_case(cuda, 5, 100, 16, 80, torch.float32, seed=3)
    anc[2, 17] = 99                                                     # outside the 8 cache rows
    out = Fn.lm_decode_attn(q, kv, anc, 100, 16, 80)
    bad = ~torch.isfinite(out).all(dim=1)
    assert bad.tolist() == [False, False, True, False, False]


# ------------------------------------------------------------------------------------------------------------------------------
# 3. incremental = full prefix, under beam reorders (duplicated parents) and a batch shrink
# ------------------------------------------------------------------------------------------------------------------------------
def _incremental_vs_full(lm, dev, rows, vocab, steps, seed, tol):
    g = torch.Generator().manual_seed(seed)
    state = lm.init_decode(rows, steps + 2)
    toks = torch.full((rows, 1), 2, dtype=torch.long)
    worst = 0.0
    for s in range(steps):
        if s > 0:
            n = rows // 2 if s == steps // 2 else rows                   # the batch shrinks half-way
            order = torch.randint(0, rows, (n,), generator=g)
            order[: n // 2] = order[0]                                    # duplicated parents
            lm.reorder(state, order.to(dev))
            toks = toks[order]
            rows = n
            toks = torch.cat([toks, torch.randint(4, vocab, (rows, 1), generator=g)], 1)
        inc = lm.decode_step(toks[:, -1].to(dev), state).float()
        full = lm(toks.to(dev))[0][:, -1]
        err = (inc - full).abs().max().item()
        scale = max(1.0, full.abs().max().item())
        worst = max(worst, err / scale)
        assert err <= tol * scale, (s, err, scale)
    return worst


def test_incremental_equals_full_prefix_tiny(cuda, fx):
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    _incremental_vs_full(_tiny_lm(fx, cuda), cuda, 10, fx["lm"]["vocab"], 40, seed=1, tol=2e-5)


def test_incremental_equals_full_prefix_real_size(cuda, real_lm):
    _incremental_vs_full(real_lm, cuda, 10, 83, 40, seed=2, tol=5e-5)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. forward() vs tests/lm_reference.py
# ------------------------------------------------------------------------------------------------------------------------------
def _vs_reference(lm, tokens, heads, dev):
    sd = {k: v.detach() for k, v in lm.state_dict().items()}
    logits, extra = lm(tokens.to(dev))
    r64, s64 = lm_forward({k: v.double() for k, v in sd.items()}, tokens.to(dev), heads)
    r32, s32 = lm_forward({k: v.float() for k, v in sd.items()}, tokens.to(dev), heads)
    pairs = [(extra["inner_states"][i].transpose(0, 1), s64[i], s32[i]) for i in range(len(s64))] + [(logits, r64, r32)]
    for i, (got, ref, ref32) in enumerate(pairs):
        e32 = (ref32.double() - ref).abs().max().item()
        err = (got.double() - ref).abs().max().item()
        assert err <= 4 * e32 + 1e-6 * max(1.0, ref.abs().max().item()), (i, err, e32)


def test_forward_matches_reference_real_size(cuda, real_lm):
    g = torch.Generator().manual_seed(5)
    toks = torch.randint(4, 83, (2, 16), generator=g)
    toks[:, 0] = 2
    toks[1, 12:] = 1                                                      # right padding
    _vs_reference(real_lm, toks, 16, cuda)


def test_forward_matches_reference_long_tiny(cuda, fx):
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    lm = _tiny_lm(fx, cuda)
    b = fx["batches"]["long"]
    assert b["tokens"].shape[1] > 1026
    _vs_reference(lm, b["tokens"], 2, cuda)
    a, z = b["keep"]
    logits = lm(b["tokens"].to(cuda))[0][:, a:z].cpu()
    assert (logits - b["logits"]).abs().max().item() <= 1e-4 * max(1.0, b["logits"].abs().max().item())
    p = fx["batches"]["padded"]
    logits = lm(p["tokens"].to(cuda))[0].cpu()
    assert (logits - p["logits"]).abs().max().item() <= 1e-4 * max(1.0, p["logits"].abs().max().item())


# ------------------------------------------------------------------------------------------------------------------------------
# 5. st5_lm_fuse_logprobs
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("w", [0.0, 0.3, 1.0])
def test_fuse_logprobs(cuda, w, ldt):
    from speecht5_amd import functional as Fn
    g = torch.Generator().manual_seed(11)
    rows, V, V_lm = 7, 36, 34
    lp = torch.log_softmax(torch.randn(rows, V, generator=g) * 3, -1)
    lp[1, 5] = lp[3, 33] = lp[2, 0] = float("-inf")
    lp[:, 35] = float("-inf")
    logits = torch.randn(rows, V_lm, generator=g) * 4
    logits[4] = torch.linspace(-80, 80, V_lm)                             # extreme range
    logits[5] = 80.0
    logits[6, ::2] = -80.0
    logits = logits.to(ldt)
    want = lp.clone()
    want[:, :V_lm] += (torch.log_softmax(logits.double(), -1) * w).float()
    got = lp.to(cuda)
    Fn.lm_fuse_logprobs(got, logits.to(cuda), w)
    got = got.cpu()
    assert torch.equal(got[:, V_lm:], lp[:, V_lm:]), "columns >= V_lm must not be touched"
    assert torch.equal(torch.isinf(got), torch.isinf(lp)) and (got[torch.isinf(lp)] < 0).all()
    if w == 0.0:
        assert torch.equal(got, lp)
    fin = torch.isfinite(want)
    assert ((got[fin] - want[fin]).abs() <= 1e-6 * want[fin].abs() + 4e-6 * max(1.0, w * 160)).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 6. bf16 compute mode
# ------------------------------------------------------------------------------------------------------------------------------
def test_bf16_log_probs_close_to_fp32(cuda, real_lm):
    from speecht5_amd import functional as Fn
    g = torch.Generator().manual_seed(8)
    toks = torch.randint(4, 83, (3, 12), generator=g).to(cuda)
    toks[:, 0] = 2
    try:
        Fn.set_compute_dtype(torch.float32)
        ref = real_lm.get_normalized_probs(real_lm(toks), log_probs=True)
        Fn.set_compute_dtype(torch.bfloat16)
        got = real_lm.get_normalized_probs(real_lm(toks), log_probs=True)
        state = real_lm.init_decode(3, 14)
        inc = []
        for s in range(12):
            inc.append(torch.log_softmax(real_lm.decode_step(toks[:, s], state).float(), -1))
        inc = torch.stack(inc, 1)
    finally:
        Fn.set_compute_dtype(torch.float32)
    bar = 0.05 * max(1.0, ref.abs().max().item())
    assert (got - ref).abs().max().item() <= bar
    assert (inc - ref).abs().max().item() <= bar


# ------------------------------------------------------------------------------------------------------------------------------
# 7. state-dict layout and conversion of a fairseq-layout module (what fairseq-generate hands over for --lm-path)
# ------------------------------------------------------------------------------------------------------------------------------
class _FairseqLayoutLM(nn.Module):
    """A plain module with fairseq transformer_lm's parameter names (no HIP code)."""

    def __init__(self, V, d, heads, layers, ffn, **opts):
        super().__init__()
        self.args = Namespace(decoder_embed_dim=d, decoder_attention_heads=heads, decoder_layers=layers, decoder_ffn_embed_dim=ffn,
                              activation_fn="gelu", **opts)
        dec = nn.Module()
        dec.embed_tokens = nn.Embedding(V, d, padding_idx=1)
        dec.register_buffer("version", torch.Tensor([3]))
        pe = nn.Module()
        pe.register_buffer("_float_tensor", torch.FloatTensor(1))
        dec.embed_positions = pe
        dec.layers = nn.ModuleList()
        for _ in range(layers):
            lay = nn.Module()
            lay.self_attn = nn.Module()
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                setattr(lay.self_attn, n, nn.Linear(d, d))
            lay.self_attn_layer_norm, lay.final_layer_norm = nn.LayerNorm(d), nn.LayerNorm(d)
            lay.fc1, lay.fc2 = nn.Linear(d, ffn), nn.Linear(ffn, d)
            dec.layers.append(lay)
        dec.layer_norm = nn.LayerNorm(d)
        dec.output_projection = nn.Linear(d, V, bias=False)
        self.decoder = dec
        with torch.no_grad():
            for n, p in self.named_parameters():
                if "layer_norm" in n:
                    p.uniform_(0.5, 1.5) if n.endswith("weight") else p.uniform_(-0.2, 0.2)


def _task():
    from speecht5_amd.task import SpeechT5Task
    return SpeechT5Task(Namespace(ctc_weight=0.0), {"text": Task().dicts["text"], "hubert": Task().dicts["hubert"]})


def test_state_dict_keys_are_fairseqs(cuda):
    from speecht5_amd.transformer_lm import TransformerLanguageModel
    torch.manual_seed(0)
    fake = _FairseqLayoutLM(34, 160, 2, 2, 320)
    lm = TransformerLanguageModel(Namespace(decoder_embed_dim=160, decoder_attention_heads=2, decoder_layers=2, decoder_ffn_embed_dim=320),
                                  vocab=34, pad=1)
    assert set(lm.state_dict()) == set(fake.state_dict())
    assert float(lm.state_dict()["decoder.version"][0]) == 3.0


def test_build_generator_converts_fairseq_lm(cuda):
    from speecht5_amd.transformer_lm import TransformerLanguageModel
    torch.manual_seed(0)
    model, _ = build_tiny(cuda, torch.float32)
    fake = _FairseqLayoutLM(34, 160, 2, 2, 320)
    gen = _task().build_generator([model], Namespace(beam=3), extra_gen_cls_kwargs={"lm_model": fake, "lm_weight": 0.5})
    lm = gen.lm_model
    assert isinstance(lm, TransformerLanguageModel) and lm.num_heads == 2
    assert next(lm.parameters()).device.type == "cuda"
    toks = torch.tensor([[2, 5, 9, 11, 4, 30, 7], [2, 8, 8, 6, 1, 1, 1]])
    got = lm(toks.to(cuda))[0].double().cpu()
    ref, _ = lm_forward({k: v.double() for k, v in fake.state_dict().items()}, toks, 2)
    assert (got - ref).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item())
    # any other LM object passes through untouched (and the generator keeps calling it on the full prefix)
    for other in (nn.Linear(4, 4), lm):
        assert _task().build_generator([model], Namespace(beam=3), extra_gen_cls_kwargs={"lm_model": other}).lm_model is other


@pytest.mark.parametrize("opt", [dict(decoder_learned_pos=True), dict(adaptive_softmax_cutoff="10,20"), dict(layernorm_embedding=True),
                                 dict(decoder_normalize_before=False), dict(no_decoder_final_norm=True), dict(character_embeddings=True),
                                 dict(decoder_input_dim=96)])
def test_unsupported_options_raise(cuda, opt):
    model, _ = build_tiny(cuda, torch.float32)
    fake = _FairseqLayoutLM(34, 160, 2, 2, 320, **opt)
    name = next(iter(opt))
    with pytest.raises(NotImplementedError, match=name):
        _task().build_generator([model], Namespace(beam=3), extra_gen_cls_kwargs={"lm_model": fake})


def test_unsupported_state_dict_layouts_raise():
    from speecht5_amd.transformer_lm import TransformerLanguageModel
    torch.manual_seed(0)
    sd = _FairseqLayoutLM(34, 160, 2, 2, 320).state_dict()
    args = Namespace(decoder_attention_heads=2)
    for extra, name in (("decoder.embed_positions.weight", "decoder_learned_pos"), ("decoder.layernorm_embedding.weight", "layernorm_embedding"),
                        ("decoder.adaptive_softmax.tail.0.weight", "adaptive_softmax")):
        bad = dict(sd)
        bad[extra] = torch.zeros(3)
        with pytest.raises(NotImplementedError, match=name):
            TransformerLanguageModel.from_state_dict(bad, args)
    bad = {k: v for k, v in sd.items() if not k.startswith("decoder.layer_norm.")}
    with pytest.raises(NotImplementedError, match="no_decoder_final_norm"):
        TransformerLanguageModel.from_state_dict(bad, args)
