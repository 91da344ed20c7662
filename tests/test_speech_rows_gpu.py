"""Length-exact batched speech encoding on the HIP kernels: st5_conv0_gn_gelu_fwd_rows, SpeechEncoderPrenet.forward_rows,
T5TransformerModel.forward_encoder_rows and what calls them (generate_speech_batch, generate_class, SequenceGenerator).

1. conv layer 0: statistics and the row's own frames bit-equal to the single-row call, zeros behind them, in every launch form;
2. tiny model fp32: the padded batch against forward_encoder on each unpadded clip (1e-5) and the CPU oracle (1e-3);
3. negative control: the reference's padded forward_encoder does NOT give the single-clip results;
4. the layer-norm extractor; 5. chunking and row permutation; 6. bf16 against the fp32 single-row call; 7. end users; 8. errors.

Measured on MI355X (profiles/speech_rows_parity.txt): see the docstrings of tests 5 and 6."""
import os
from argparse import Namespace
from types import SimpleNamespace

import pytest
import torch

from tests import speech_rows_reference as R
from tests.util import G, Task, build_tiny, close, load_golden

pytestmark = pytest.mark.gpu

MARGIN = 1e-4          # (tests/test_tts_batch_gpu.py: the distance a decision must keep from its threshold to be compared)
K0, S0 = 10, 5         # conv layer 0 of every recipe
TCM = 1024             # frames per block of the moments pass (csrc/conv0.hip)


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


def _report(line):
    """Printed, and appended to the file ST5_PARITY_OUT names (how profiles/speech_rows_parity.txt was written)."""
    print(line)
    path = os.environ.get("ST5_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _batch(lengths, cuda, seed=1, fill=0.0):
    wav, pad, clips = R.padded_batch(lengths, seed=seed, dtype=torch.float32, fill=fill)
    return wav.to(cuda), pad.to(cuda), [c.to(cuda) for c in clips]


def _single(model, clip):
    return model.forward_encoder(clip[None, :], padding_mask=torch.zeros(1, clip.numel(), dtype=torch.bool, device=clip.device))


def _rel(a, b):
    return R.rel_err(a.double().cpu(), b.double().cpu())


# ------------------------------------------------------------------------------------------------------------------------------
# 1. conv layer 0, bits
# ------------------------------------------------------------------------------------------------------------------------------
def _l0(n):
    return (n - K0) // S0 + 1


CONV0_LENGTHS = R.LENGTHS + [40003,                         # the longest, not a multiple of 4: rows start off the 16-byte grid
                             (5000 - 1) * S0 + K0,          # 5000 frames: several moment chunks, the last one partial
                             (2 * TCM - 1) * S0 + K0]       # 2048 frames: ends exactly on a chunk boundary


def _conv0_call(wav, w, gamma, beta, dtype, lens=None, poison=7.0):
    from speecht5_amd import hip
    L = hip.lib()
    B, S = wav.shape
    C, k = w.shape
    out = torch.full((B, _l0(S), C), poison, dtype=dtype, device=wav.device)
    stats = torch.full((B, C, 2), poison, dtype=torch.float32, device=wav.device)
    ws = hip.workspace(L.st5_conv0_ws_bytes(B, S, C, k, S0), wav.device)
    if lens is None:
        hip.check(L.st5_conv0_gn_gelu_fwd(wav.data_ptr(), w.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), stats.data_ptr(),
                                          ws.data_ptr(), B, S, C, k, S0, 1e-5, hip.dt(dtype), hip.stream()), "st5_conv0_gn_gelu_fwd")
    else:
        hip.check(L.st5_conv0_gn_gelu_fwd_rows(wav.data_ptr(), lens.data_ptr(), w.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                               stats.data_ptr(), ws.data_ptr(), B, S, C, k, S0, 1e-5, hip.dt(dtype), hip.stream()),
                  "st5_conv0_gn_gelu_fwd_rows")
    torch.cuda.synchronize()
    return out, stats


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_conv0_rows_bit_equal_to_single_row_calls(cuda, dtype, fold, mfma):
    from speecht5_amd import hip
    L = hip.lib()
    C = 512
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(C, K0, generator=g) * 0.3).to(cuda)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(cuda)
    beta = (0.1 * torch.randn(C, generator=g)).to(cuda)
    lengths = CONV0_LENGTHS
    assert _l0(lengths[-1]) == 2 * TCM and _l0(lengths[-2]) > 4 * TCM and max(lengths) % 4 == 3
    wav, _, clips = _batch(lengths, cuda, seed=5, fill=0.0)
    pad_noise = torch.randn(wav.shape, generator=g).to(cuda)                      # the padding holds anything but zeros
    for b, n in enumerate(lengths):
        wav[b, n:] = 3.0 * pad_noise[b, n:]
    lens = torch.tensor(lengths, dtype=torch.int32, device=cuda)
    L.st5_conv0_set_fold(fold)
    L.st5_conv0_set_mfma(mfma)
    try:
        out, stats = _conv0_call(wav, w, gamma, beta, dtype, lens=lens)
        for b, n in enumerate(lengths):
            o1, s1 = _conv0_call(clips[b][None, :].contiguous(), w, gamma, beta, dtype)
            Lb = _l0(n)
            assert o1.shape[1] == Lb
            assert torch.equal(stats[b], s1[0]), f"row {b} ({n} samples): statistics differ from the single-row call"
            assert torch.equal(out[b, :Lb], o1[0]), f"row {b} ({n} samples): frames differ from the single-row call"
            assert bool((out[b, Lb:] == 0).all()), f"row {b} ({n} samples): frames behind the row's own are not zero"
        assert bool(torch.isfinite(out.float()).all())
    finally:
        L.st5_conv0_set_fold(1)
        L.st5_conv0_set_mfma(1)


def test_conv0_rows_same_statistics_in_every_launch_form(cuda):
    from speecht5_amd import hip
    L = hip.lib()
    C = 512
    g = torch.Generator().manual_seed(12)
    w = (torch.randn(C, K0, generator=g) * 0.3).to(cuda)
    gamma, beta = torch.ones(C, device=cuda), torch.zeros(C, device=cuda)
    wav, _, _ = _batch(CONV0_LENGTHS, cuda, seed=6)
    lens = torch.tensor(CONV0_LENGTHS, dtype=torch.int32, device=cuda)
    got = []
    try:
        for fold in (0, 1):
            for mfma in (0, 1):
                L.st5_conv0_set_fold(fold)
                L.st5_conv0_set_mfma(mfma)
                got.append(_conv0_call(wav, w, gamma, beta, torch.bfloat16, lens=lens)[1])
    finally:
        L.st5_conv0_set_fold(1)
        L.st5_conv0_set_mfma(1)
    assert all(torch.equal(got[0], s) for s in got[1:])


# ------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. pre-net and encoder, tiny model
# ------------------------------------------------------------------------------------------------------------------------------
def _tiny(cuda, dtype=torch.float32):
    model, args = build_tiny(cuda, dtype)
    return model.eval(), args


def _check_rows(enc, singles, frames_of, tol, what):
    x, mask = enc["encoder_out"][0], enc["encoder_padding_mask"][0]
    assert x.size(0) == max(frames_of) and tuple(mask.shape) == (len(singles), x.size(0))
    for b, s in enumerate(singles):
        one = s["encoder_out"][0]
        T = one.size(0)
        assert T == frames_of[b], (b, T, frames_of[b])
        assert mask[b].tolist() == [False] * T + [True] * (x.size(0) - T), f"{what}: row {b} mask"
        close(x[:T, b], one[:, 0], tol, what=f"{what}: row {b}")


def test_tiny_rows_match_single_clips_and_oracle(cuda):
    from oracle import speecht5_oracle as O
    model, _ = _tiny(cuda)
    wav, pad, clips = _batch(R.LENGTHS, cuda)
    m, _ = load_golden(None)
    sd = {k: v.detach().float() for k, v in m["state_dict"].items()}
    cfg = SimpleNamespace(**m["args"])
    frames_of = [R.frames(n, R.layers_of(cfg)) for n in R.LENGTHS]
    with torch.no_grad():
        enc = model.forward_encoder_rows(wav, padding_mask=pad)
        singles = [_single(model, c) for c in clips]
        _check_rows(enc, singles, frames_of, 1e-5, "rows vs single clip")
        enc2 = model.forward_encoder_rows(wav, src_lengths=R.LENGTHS)
        assert torch.equal(enc2["encoder_out"][0], enc["encoder_out"][0])
        x = enc["encoder_out"][0]
        for b, c in enumerate(clips):
            pm = torch.zeros(1, c.numel(), dtype=torch.bool)
            pre = O.speech_encoder_prenet(sd, cfg, c.cpu()[None, :], pm)
            ref = O.encoder(sd, cfg, pre["x"], pre["padding_mask"])["encoder_out"][0]
            close(x[:frames_of[b], b], ref[:, 0], 1e-3, what=f"rows vs oracle: row {b}")


def test_negative_control_padded_forward_encoder_differs(cuda):
    """Why the feature exists: the reference's padded batch gives a shorter row something else than the row alone gets.  The lengths
    are those for which tests/test_speech_rows_cpu.py shows 0.1 ... 0.18 relative in the pre-net already."""
    model, _ = _tiny(cuda)
    lengths = [16000, 40000, 27200]
    wav, pad, clips = _batch(lengths, cuda)
    with torch.no_grad():
        x = model.forward_encoder(wav, padding_mask=pad)["encoder_out"][0]
        errs = []
        for b, c in enumerate(clips):
            one = _single(model, c)["encoder_out"][0]
            errs.append(_rel(x[:one.size(0), b], one[:, 0]))
    print("padded forward_encoder vs single clips:", " ".join(f"{e:.2e}" for e in errs))
    assert errs[1] <= 1e-5                      # the longest row has no padding
    assert max(errs[0], errs[2]) > 1e-3


# ------------------------------------------------------------------------------------------------------------------------------
# 4. layer-norm extractor
# ------------------------------------------------------------------------------------------------------------------------------
def test_layer_norm_extractor_rows_match_single_clips_and_oracle(cuda):
    from oracle import speecht5_oracle as O
    from speecht5_amd import functional as Fn
    from speecht5_amd.speecht5 import T5TransformerModel
    fx = torch.load(os.path.join(G, "tiny_large_speech_pretrain.pt"), weights_only=False)
    args = Namespace(**fx["args"])
    assert args.extractor_mode == "layer_norm"
    Fn.set_compute_dtype(torch.float32)
    model = T5TransformerModel.build_model(args, Task())
    torch.nn.Module.load_state_dict(model, fx["state_dict"], strict=True)
    model = model.to(cuda).eval()
    layers = eval(args.conv_feature_layers)
    lengths = [16000, 40000, 27200, model.speech_encoder_prenet.min_samples(), 16079, 16080]
    frames_of = [R.frames(n, layers) for n in lengths]
    wav, pad, clips = _batch(lengths, cuda, seed=2, fill=0.25)
    sd = {k: v.detach().float() for k, v in fx["state_dict"].items()}
    cfg = SimpleNamespace(**fx["args"])
    with torch.no_grad():
        enc = model.forward_encoder_rows(wav, padding_mask=pad)
        singles = [_single(model, c) for c in clips]
        _check_rows(enc, singles, frames_of, 1e-5, "layer_norm rows vs single clip")
        x = enc["encoder_out"][0]
        for b, c in enumerate(clips):
            pre = O.speech_encoder_prenet(sd, cfg, c.cpu()[None, :], torch.zeros(1, c.numel(), dtype=torch.bool))
            ref = O.encoder(sd, cfg, pre["x"], pre["padding_mask"])["encoder_out"][0]
            close(x[:frames_of[b], b], ref[:, 0], 1e-3, what=f"layer_norm rows vs oracle: row {b}")


# ------------------------------------------------------------------------------------------------------------------------------
# 5. chunking, row permutation
# ------------------------------------------------------------------------------------------------------------------------------
def _valid_rows(enc, frames_of):
    x = enc["encoder_out"][0]
    return [x[:T, b] for b, T in enumerate(frames_of)]


def test_two_chunks_and_row_permutation(cuda):
    """fp32, 1e-5.  Whether the rows come out bit-equal is recorded per case (profiles/speech_rows_parity.txt) and NOT asserted."""
    dtype = torch.float32
    model, args = _tiny(cuda, dtype)
    layers = eval(args.conv_feature_layers)
    frames_of = [R.frames(n, layers) for n in R.LENGTHS]
    wav, pad, _ = _batch(R.LENGTHS, cuda)
    tol, name = 1e-5, "fp32"
    with torch.no_grad():
        limit = 3 * max(R.LENGTHS)
        assert model._plan_row_chunks(R.LENGTHS, limit) == [[0, 1, 2], [3, 4, 5]]
        assert model._plan_row_chunks(R.LENGTHS, None) == [[0, 1, 2, 3, 4, 5]]
        one = model.forward_encoder_rows(wav, padding_mask=pad)
        two = model.forward_encoder_rows(wav, padding_mask=pad, max_samples=limit)
        assert torch.equal(one["encoder_padding_mask"][0], two["encoder_padding_mask"][0])
        a, b = _valid_rows(one, frames_of), _valid_rows(two, frames_of)
        for r in range(len(a)):
            close(b[r], a[r], tol, what=f"two chunks vs one: row {r}")
        _report(f"chunking {name}: two chunks vs one, rows bit-equal: {[bool(torch.equal(p, q)) for p, q in zip(a, b)]}")
        perm = [4, 2, 0, 5, 1, 3]
        pwav, ppad, _ = _batch([R.LENGTHS[i] for i in perm], cuda)
        for i, src in enumerate(perm):
            pwav[i] = wav[src]
        got = _valid_rows(model.forward_encoder_rows(pwav, padding_mask=ppad), [frames_of[i] for i in perm])
        for i, src in enumerate(perm):
            close(got[i], a[src], tol, what=f"permuted row {i} (row {src})")
        _report(f"permutation {name}: permuted vs original, rows bit-equal: {[bool(torch.equal(got[i], a[src])) for i, src in enumerate(perm)]}")


# ------------------------------------------------------------------------------------------------------------------------------
# 6. bf16
# ------------------------------------------------------------------------------------------------------------------------------
def test_bf16_rows_no_worse_than_bf16_single_clips(cuda):
    """Reference: the fp32 single-clip call.  Per row, max-norm relative: the batched bf16 error may be at most 1.5 x the single-clip
    bf16 error (the margin covers another GEMM tile choice at another M)."""
    lengths = R.LENGTHS
    wav, pad, clips = _batch(lengths, cuda)
    model, _ = _tiny(cuda, torch.float32)
    with torch.no_grad():
        ref = [_single(model, c)["encoder_out"][0][:, 0].float().clone() for c in clips]
    del model
    model, _ = _tiny(cuda, torch.bfloat16)
    with torch.no_grad():
        x = model.forward_encoder_rows(wav, padding_mask=pad)["encoder_out"][0]
        ones = [_single(model, c)["encoder_out"][0][:, 0] for c in clips]
    bad = []
    for b, n in enumerate(lengths):
        T = ref[b].size(0)
        eb, es = _rel(x[:T, b], ref[b]), _rel(ones[b], ref[b])
        same = bool(torch.equal(x[:T, b], ones[b]))
        _report(f"bf16 row {b} ({n} samples, {T} frames): batched {eb:.3e}  single {es:.3e}  ratio {eb / max(es, 1e-30):.3f}  bit-equal {same}")
        if eb > 1.5 * es:
            bad.append((b, eb, es))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------------
# 7. end users
# ------------------------------------------------------------------------------------------------------------------------------
def test_generate_class_exact_rows_gives_single_clip_classes(cuda):
    from tests.test_sid_gpu import _tiny as sid_tiny
    fx = torch.load(os.path.join(G, "tiny_s2c.pt"), weights_only=False)
    model = sid_tiny(fx, "recipe", cuda, torch.float32).eval()
    ni = fx["sample"]["net_input"]
    lengths = [6000, 4321, 2500]
    src = ni["source"].to(cuda).clone()
    pad = torch.ones(src.shape, dtype=torch.bool, device=cuda)
    for b, n in enumerate(lengths):
        pad[b, :n] = False
        src[b, n:] = 0
    prev = ni["prev_output_tokens"].to(cuda)
    seen = []
    hook = model.speaker_decoder_postnet.register_forward_hook(lambda m, i, o: seen.append(o[0].detach().float().cpu()))
    try:
        want, keep = [], []
        for b, n in enumerate(lengths):
            c = model.generate_class(src[b:b + 1, :n], prev[b:b + 1], padding_mask=torch.zeros(1, n, dtype=torch.bool, device=cuda))
            top = seen[-1][0].topk(2).values
            want.append(int(c[0]))
            if float(top[0] - top[1]) > 1e-3:
                keep.append(b)
    finally:
        hook.remove()
    assert len(keep) >= 2, f"top-two logit gaps leave rows {keep} only"
    got = model.generate_class(src, prev, padding_mask=pad, exact_rows=True)
    assert got.dtype == torch.int64
    assert [int(got[b]) for b in keep] == [want[b] for b in keep]


def _step_margin(model, gen, enc_single, hyp):
    """Smallest gap between the best and the second-best candidate at the steps of the single-clip best hypothesis (teacher-forced
    through the decoder, the generator's banned symbols removed), the step at which the length limit forces eos left out."""
    toks = hyp["tokens"]
    prefix = torch.cat([toks.new_full((1,), gen.eos), toks[:-1]])[None, :]
    logits, _ = model.forward_decoder(prefix, encoder_out=enc_single, incremental_state=None)
    lp = model.get_normalized_probs((logits, None), log_probs=True, sample=None)[0].float()
    lp[:, gen.pad] = float("-inf")
    lp = gen._never(lp)
    lp[:gen.min_len, gen.eos] = float("-inf")
    top = lp.topk(2, dim=-1).values
    gaps = (top[:, 0] - top[:, 1])
    if len(toks) >= gen.max_len_b + 1:          # (the last eos was forced by the length limit: no decision)
        gaps = gaps[:-1]
    return float(gaps.min()) if gaps.numel() else float("inf")


def test_sequence_generator_exact_rows_gives_single_clip_hypotheses(cuda):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _ = _tiny(cuda)
    d = Task().dicts["text"]
    batches = {"a": [16000, 9000, 12345], "b": [8000, 16079, 11000]}
    kw = dict(max_len_a=0, max_len_b=12, ctc_weight=0.0)
    kept, results = [], {}
    for beam in (1, 4):
        for name, lengths in batches.items():
            wav, pad, clips = _batch(lengths, cuda, seed=40 + len(name) + lengths[0] % 7)
            gen = SequenceGenerator([model], d, beam_size=beam, **kw)
            singles, margin = [], float("inf")
            for c in clips:
                ni = {"source": c[None, :], "padding_mask": torch.zeros(1, c.numel(), dtype=torch.bool, device=cuda)}
                hyps = gen.generate([model], {"net_input": ni})[0]
                singles.append(hyps[0])
                with torch.no_grad():
                    margin = min(margin, _step_margin(model, gen, _single(model, c), hyps[0]))
                if len(hyps) > 1:
                    margin = min(margin, abs(float(hyps[0]["score"]) - float(hyps[1]["score"])))
            print(f"beam {beam} batch {name}: smallest single-clip margin {margin:.3e}")
            if margin > MARGIN:
                kept.append((beam, name))
            results[(beam, name)] = (wav, pad, singles)
    assert len(kept) >= 3, f"margins leave {kept} only"
    for beam, name in kept:
        wav, pad, singles = results[(beam, name)]
        gen = SequenceGenerator([model], d, beam_size=beam, exact_rows=True, **kw)
        hyps = gen.generate([model], {"net_input": {"source": wav, "padding_mask": pad}})
        for b, s in enumerate(singles):
            assert hyps[b][0]["tokens"].tolist() == s["tokens"].tolist(), f"beam {beam} batch {name} row {b}"
            assert abs(float(hyps[b][0]["score"]) - float(s["score"])) <= 2e-4 * max(1.0, abs(float(s["score"])))


def _count_rows_calls(model, fn):
    calls = []
    inner = model.forward_encoder_rows
    model.forward_encoder_rows = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    try:
        out = fn()
    finally:
        del model.forward_encoder_rows
    return out, len(calls)


def test_exact_rows_belongs_to_the_generator_and_travels_through_build_generator(cuda):
    from speecht5_amd.sequence_generator import EnsembleModel, SequenceGenerator
    from speecht5_amd.task import SpeechT5Task
    model, args = _tiny(cuda)
    d = Task().dicts["text"]
    kw = dict(max_len_a=0, max_len_b=6, ctc_weight=0.0)
    wav, pad, _ = _batch([16000, 9000, 12345], cuda, seed=41)
    sample = {"net_input": {"source": wav, "padding_mask": pad}}
    shared = EnsembleModel([model])
    exact = SequenceGenerator(shared, d, beam_size=1, exact_rows=True, **kw)
    plain = SequenceGenerator(shared, d, beam_size=1, **kw)          # built second, on the same EnsembleModel, with the default
    assert exact.exact_rows is True and plain.exact_rows is False
    h_exact, n = _count_rows_calls(model, lambda: exact.generate([model], sample))
    assert n == 1
    _, n = _count_rows_calls(model, lambda: plain.generate([model], sample))
    assert n == 0
    task = SpeechT5Task(args, Task().dicts)
    gen_args = Namespace(beam=1, max_len_a=0, max_len_b=6)
    built = task.build_generator([model], gen_args, extra_gen_cls_kwargs={"exact_rows": True})
    assert built.exact_rows is True and task.build_generator([model], gen_args).exact_rows is False
    h_built, n = _count_rows_calls(model, lambda: built.generate([model], sample))
    assert n == 1
    for a, b in zip(h_built, h_exact):
        assert a[0]["tokens"].tolist() == b[0]["tokens"].tolist()


def test_training_mode_keeps_the_per_clip_loop(cuda):
    """generate_speech_batch(source=...) on a model in training mode ran through forward_encoder per clip before the rows path
    existed; forward_rows is eval only, so that route stays."""
    model, args = _tiny(cuda)
    lengths = [16000, 40000, 27200]
    wav, pad, _ = _batch(lengths, cuda, seed=55)
    model.train()
    calls = []
    inner = model.forward_encoder
    model.forward_encoder = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    try:
        with torch.no_grad():
            enc, T = model._encode_rows(wav, None, pad)
    finally:
        del model.forward_encoder
    assert len(calls) == 3 and T == [R.frames(n, eval(args.conv_feature_layers)) for n in lengths]
    assert tuple(enc["encoder_out"][0].shape[:2]) == (max(T), 3)


def test_generate_speech_batch_makes_no_per_row_encoder_call(cuda):
    m, fx = load_golden("tiny_t2s.pt")
    spk = fx["sample"]["net_input"]["spkembs"].to(cuda)
    model, _ = _tiny(cuda)
    lengths = [16000, 40000, 27200]
    wav, pad, _ = _batch(lengths, cuda, seed=55)
    calls = []
    inner = model.forward_encoder
    model.forward_encoder = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    try:
        out = model.generate_speech_batch(source=wav, spkembs=spk, padding_mask=pad, need_attn=False)
    finally:
        del model.forward_encoder
    assert len(out) == 3 and all(bool(torch.isfinite(o[0]).all()) for o in out)
    assert calls == [], f"{len(calls)} forward_encoder calls for a batch of {len(lengths)} clips"


# ------------------------------------------------------------------------------------------------------------------------------
# 8. errors
# ------------------------------------------------------------------------------------------------------------------------------
def test_rows_path_rejects_what_it_cannot_do(cuda):
    model, _ = _tiny(cuda)
    wav, pad, _ = _batch([16000, 399], cuda)
    with torch.no_grad():
        with pytest.raises(ValueError, match="shorter than one frame"):
            model.forward_encoder_rows(wav, padding_mask=pad)
        with pytest.raises(ValueError, match="exceeds"):
            model.forward_encoder_rows(wav, src_lengths=[16000, 16001])
        holes = pad.clone()
        holes[1, :] = False
        holes[1, 100:200] = True
        with pytest.raises(ValueError, match="not a suffix"):
            model.forward_encoder_rows(wav, padding_mask=holes)
    wav, pad, _ = _batch([16000, 8000], cuda)
    assert any(p.requires_grad for p in model.parameters())
    with pytest.raises(RuntimeError, match="inference only"):
        model.forward_encoder_rows(wav, padding_mask=pad)
    model.train()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="eval"):
            model.forward_encoder_rows(wav, padding_mask=pad)
