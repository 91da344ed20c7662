"""Batched speech synthesis on the HIP kernels: T5TransformerModel.generate_speech_batch and csrc/tts_decode.hip.

1. st5_decode_cross_attn against the fp64 restatement (tests/tts_batch_reference.py) up to S = 7999 with ragged masks;
2. st5_tts_step_tail against the restatement of the stop rule;
3. the tiny golden model: the batch against the verbatim reference's mel, the CPU oracle and the single-row generate_speech, with
   rows that stop at different, data-dependent steps;
4. row permutation; 5. speech input; 6. pre-LN decoder; 7. need_attn=False; 8. pre-net dropout; 9. Base size; 10. task methods."""
from argparse import Namespace
from types import SimpleNamespace

import pytest
import torch

from tests import tts_batch_reference as R
from tests.util import Task, build_tiny, close, load_golden

pytestmark = pytest.mark.gpu

MARGIN = 1e-4


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


# ------------------------------------------------------------------------------------------------------------------------------
# 1. one-query cross-attention
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S", [1, 5, 100, 499, 4097, 7999])
@pytest.mark.parametrize("B", [1, 3, 32])
def test_cross_attn_kernel_matches_fp64(cuda, B, S, dtype):
    from speecht5_amd import functional as Fn
    H = 12 if B * S <= 40000 else 2
    hd, C, off = 64, H * 64, 8
    g = torch.Generator().manual_seed(1000 * B + S)
    q = torch.randn(B, C, generator=g).to(dtype)
    kv = (torch.randn(B * S, 2 * C + off, generator=g) * 2).to(dtype)   # [K | V] at column `off` of wider rows
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    if B > 1:
        lens[1] = 1                                                      # a row with a single valid key
    kpm = (torch.arange(S)[None, :] >= lens[:, None]).to(torch.uint8)
    cap, col = 3, 1
    rec = torch.full((B, H, cap, S), 7.0, device=cuda)
    qd, kvd, kpmd = q.to(cuda), kv.to(cuda), kpm.to(cuda)
    ctx = Fn.decode_cross_attn(qd, kvd, off, S, H, hd, kpm=kpmd, probs=(rec[:, :, col], rec.stride(0), rec.stride(1)))
    ctx2 = Fn.decode_cross_attn(qd, kvd, off, S, H, hd, kpm=kpmd)
    torch.cuda.synchronize()
    ref_ctx, ref_p = R.cross_attn(q, kv, off, S, H, hd, kpm)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    close(ctx, ref_ctx, tol, what=f"ctx B={B} S={S}")
    assert torch.equal(ctx, ctx2), "ctx depends on the probability write"
    p = rec[:, :, col].cpu()
    close(p, ref_p, 1e-5 if dtype == torch.float32 else 2e-2, what="probabilities")
    masked = kpm.bool()[:, None, :].expand(B, H, S)
    assert (p[masked] == 0).all(), "masked keys must get probability exactly 0"
    assert (p.double().sum(-1) - 1).abs().max() < 1e-4
    others = torch.cat([rec[:, :, :col], rec[:, :, col + 1:]], dim=2)
    assert (others == 7.0).all(), "record columns other than the step's were written"


def test_cross_attn_kernel_rejects_other_head_dims(cuda):
    from speecht5_amd import functional as Fn
    from speecht5_amd.hip import HipKernelError
    q = torch.zeros(2, 160, device=cuda)
    kv = torch.zeros(2 * 4, 320, device=cuda)
    with pytest.raises(HipKernelError):
        Fn.decode_cross_attn(q, kv, 0, 4, 2, 80)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. step tail
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_step_tail_matches_restatement(cuda, dtype):
    from speecht5_amd import functional as Fn
    B, r, odim, cap, idx, thr = 7, 2, 80, 5, 3, 0.5
    g = torch.Generator().manual_seed(7)
    y = torch.randn(B, r * odim + r + 3, generator=g)          # (a wider row stride than r*odim + r)
    lo = -3.0
    y[:, r * odim:r * odim + r] = lo
    minlen = torch.tensor([0, 4, 0, 0, 0, 0, 3], dtype=torch.int32)
    maxlen = torch.tensor([9, 9, 3, 9, 9, 9, 2], dtype=torch.int32)
    y[0, r * odim + 1] = 0.0        # probability exactly the threshold: stops
    y[1, r * odim] = 4.0            # above the threshold, but idx < minlen: held back
    #   row 2: low probabilities, idx >= maxlen: forced stop
    done = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.int32)    # row 3 finished earlier: nothing of it is written
    steps = torch.tensor([0, 0, 0, 2, 0, 0, 0], dtype=torch.int32)
    #   row 4: keeps running
    y[5, r * odim] = 0.7            # first of the r probabilities above: stops
    #   row 6: minlen 3 == idx, maxlen 2 < idx: stops on the length
    mel = torch.full((B, cap * r, odim), -5.0)
    probs = torch.full((B, cap * r), -5.0)
    nxt = torch.full((B, odim), -5.0).to(dtype)
    dev = [t.to(cuda) for t in (y, minlen, maxlen, done, steps, mel, probs, nxt)]
    active = torch.full((1,), -1, dtype=torch.int32, device=cuda)
    Fn.tts_step_tail(dev[0], r, odim, dev[1], dev[2], dev[3], dev[4], idx, thr, dev[5], dev[6], dev[7], active)
    torch.cuda.synchronize()
    want_n = R.step_tail(y, r, odim, minlen, maxlen, done, steps, idx, thr, mel, probs, nxt)
    assert done.tolist() == [1, 0, 1, 1, 0, 1, 1] and steps.tolist() == [3, 0, 3, 2, 0, 3, 3]
    assert int(active) == want_n == 2
    assert torch.equal(dev[3].cpu(), done) and torch.equal(dev[4].cpu(), steps)
    assert torch.equal(dev[5].cpu(), mel)
    close(dev[6].cpu(), probs, 1e-6, what="stop probabilities")
    assert (dev[6].cpu()[3] == -5.0).all() and (dev[5].cpu()[3] == -5.0).all()
    assert torch.equal(dev[7].cpu(), nxt)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. tiny golden model
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    m, fx = load_golden("tiny_t2s.pt")
    ni = fx["sample"]["net_input"]
    sd = {k: v.detach().float() for k, v in m["state_dict"].items()}
    return SimpleNamespace(fx=fx, toks=ni["src_tokens"], spk=ni["spkembs"], lens=ni["src_lengths"].tolist(), sd=sd,
                           cfg=SimpleNamespace(**m["args"]))


def _tiny(cuda, dtype=torch.float32):
    model, args = build_tiny(cuda, dtype)
    model.eval()
    return model, args


def _singles(model, toks, spk, lens, **kw):
    return [model.generate_speech(src_tokens=toks[b:b + 1, :lens[b]], spkembs=spk[b:b + 1], **kw) for b in range(len(lens))]


def _assert_margin(probs, thr, what):
    m = float((probs.float() - thr).abs().min())
    assert m > MARGIN, f"{what}: a stop probability lies {m:.2e} from the threshold"


def _same_as_single(out, singles, tol=1e-5):
    for b, (got, ref) in enumerate(zip(out, singles)):
        assert got[0].shape == ref[0].shape, (b, got[0].shape, ref[0].shape)
        close(got[0], ref[0], tol, what=f"row {b} mel")
        close(got[1], ref[1], tol, what=f"row {b} probs")
        assert got[2].shape == ref[2].shape, (b, got[2].shape, ref[2].shape)
        close(got[2], ref[2], tol, what=f"row {b} attn")


def test_tiny_golden_batch_matches_reference_oracle_and_single_rows(cuda, golden):
    from oracle import speecht5_oracle as O
    model, _ = _tiny(cuda)
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    out = model.generate_speech_batch(src_tokens=toks, spkembs=spk)
    close(out[0][0], golden.fx["generated_mel"], 1e-3, what="row 0 vs the verbatim reference's generated mel")
    singles = _singles(model, toks, spk, golden.lens)
    for b, s in enumerate(singles):
        _assert_margin(s[1], 0.5, f"row {b}")
    _same_as_single(out, singles)
    with torch.no_grad():
        for b in range(3):
            ref = O.generate_speech(golden.sd, golden.cfg, golden.toks[b:b + 1, :golden.lens[b]], golden.spk[b:b + 1])
            assert out[b][0].shape == ref.shape == singles[b][0].shape
            close(out[b][0], ref, 1e-3, what=f"row {b} vs the oracle")


def _pick_stop_shift(singles, r, maxlen):
    """A shift of the stop logits under which the rows stop at different steps: as many of them as possible on their stop
    probability before maxlen, then as many distinct steps and as late a first stop as possible.  The shift lies midway between two adjacent distinct stop logits of the unshifted runs, at least
    1e-3 from each (a probability margin > 2.5e-4 around 0.5).  The stop logits do not feed back into the decode, so the unshifted
    trajectories give every row's stopping step for any shift."""
    z = [torch.logit(s[1].double().cpu()).view(-1, r) for s in singles]
    vals = torch.cat([zb.flatten() for zb in z]).unique()
    vals = vals[torch.isfinite(vals)].sort(descending=True).values.tolist()
    best = None
    for a, c in zip(vals[:-1], vals[1:]):
        if a - c < 2e-3:
            continue
        shift = -(a + c) / 2
        stops = []
        for zb, ml in zip(z, maxlen):
            hit = (zb.max(1).values + shift >= 0).nonzero()
            stops.append(min(int(hit[0]) + 1, ml) if len(hit) else ml)
        score = (sum(s < ml for s, ml in zip(stops, maxlen)), len(set(stops)), min(stops))
        if score[0] > 0 and score[1] >= 2 and (best is None or score > best[2]):
            best = (shift, stops, score)
    assert best is not None, "no stop-logit shift separates the rows"
    return best[0], best[1]


def test_tiny_rows_stop_at_different_data_dependent_steps(cuda, golden):
    from speecht5_amd import functional as Fn
    model, args = _tiny(cuda)
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    maxlen = [int(n * 20.0 / args.reduction_factor) for n in golden.lens]
    shift, stops = _pick_stop_shift(_singles(model, toks, spk, golden.lens), args.reduction_factor, maxlen)
    with torch.no_grad():
        model.speech_decoder_postnet.prob_out.bias.add_(shift)    # lowered when the rows would otherwise never stop
    Fn.weight_cache.clear()
    singles = _singles(model, toks, spk, golden.lens)
    out = model.generate_speech_batch(src_tokens=toks, spkembs=spk)
    lens = [o[0].shape[0] // args.reduction_factor for o in out]
    print(f"stop-logit shift {shift:+.4f}: steps {lens} (predicted {stops}, maxlen {maxlen})")
    for b, s in enumerate(singles):
        _assert_margin(s[1], 0.5, f"row {b}")
    _same_as_single(out, singles)
    assert lens == stops
    assert len(set(lens)) >= 2
    assert any(n < ml and bool((o[1] >= 0.5).any()) for n, ml, o in zip(lens, maxlen, out))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. row permutation
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_row_permutation_is_bit_identical(cuda, golden, dtype):
    model, _ = _tiny(cuda, dtype)
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    perm = [2, 0, 1]
    out = model.generate_speech_batch(src_tokens=toks, spkembs=spk)
    outp = model.generate_speech_batch(src_tokens=toks[perm], spkembs=spk[perm])
    for i, b in enumerate(perm):
        for k in range(3):
            assert torch.equal(outp[i][k], out[b][k]), (i, b, k)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. speech input
# ------------------------------------------------------------------------------------------------------------------------------
def test_speech_rows_match_single_clip_calls(cuda, golden):
    model, _ = _tiny(cuda)
    g = torch.Generator().manual_seed(55)
    n = [16000, 40000, 27200]                                    # 1.0 s, 2.5 s, 1.7 s
    src = torch.zeros(3, max(n))
    pad = torch.ones(3, max(n), dtype=torch.bool)
    for b, m in enumerate(n):
        src[b, :m] = torch.randn(m, generator=g) * 0.1
        pad[b, :m] = False
    src, pad, spk = src.to(cuda), pad.to(cuda), golden.spk.to(cuda)
    out = model.generate_speech_batch(source=src, spkembs=spk, padding_mask=pad)
    singles = [model.generate_speech(source=src[b:b + 1, :m], spkembs=spk[b:b + 1],
                                     padding_mask=torch.zeros(1, m, dtype=torch.bool, device=cuda)) for b, m in enumerate(n)]
    for b, s in enumerate(singles):
        _assert_margin(s[1], 0.5, f"speech row {b}")
    _same_as_single(out, singles)
    assert len({o[2].shape[-1] for o in out}) == 3          # three different encoder lengths


# ------------------------------------------------------------------------------------------------------------------------------
# 6. pre-LN decoder
# ------------------------------------------------------------------------------------------------------------------------------
def test_pre_ln_decoder_matches_single_rows(cuda, golden):
    from speecht5_amd import functional as Fn
    from speecht5_amd.speecht5 import T5TransformerModel
    m, _ = load_golden(None)
    args = Namespace(**dict(m["args"], decoder_normalize_before=True))
    Fn.set_compute_dtype(torch.float32)
    torch.manual_seed(3)
    model = T5TransformerModel.build_model(args, Task())
    torch.nn.Module.load_state_dict(model, m["state_dict"], strict=False)
    with torch.no_grad():
        model.decoder.layer_norm.weight.uniform_(0.5, 1.5)
        model.decoder.layer_norm.bias.uniform_(-0.1, 0.1)
    model = model.to(cuda).eval()
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    out = model.generate_speech_batch(src_tokens=toks, spkembs=spk)
    singles = _singles(model, toks, spk, golden.lens)
    _same_as_single(out, singles)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. need_attn=False, 8. pre-net dropout
# ------------------------------------------------------------------------------------------------------------------------------
def test_need_attn_off_gives_same_bits_and_no_record(cuda, golden):
    model, _ = _tiny(cuda)
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    on = model.generate_speech_batch(src_tokens=toks, spkembs=spk)
    off = model.generate_speech_batch(src_tokens=toks, spkembs=spk, need_attn=False)
    for a, b in zip(on, off):
        assert b[2] is None and a[2] is not None
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_prenet_dropout_draws_per_row(cuda, golden):
    model, _ = _tiny(cuda)
    toks, spk = golden.toks[[0, 0]].to(cuda), golden.spk[[0, 0]].to(cuda)
    tac = model.speech_decoder_prenet.decoder_prenet[0][0]
    same = model.generate_speech_batch(src_tokens=toks, spkembs=spk, threshold=1.0, need_attn=False)
    assert torch.equal(same[0][0], same[1][0])
    tac.dropout_rate = 0.5
    try:
        diff = model.generate_speech_batch(src_tokens=toks, spkembs=spk, threshold=1.0, need_attn=False)
    finally:
        tac.dropout_rate = 0.0
    assert all(bool(torch.isfinite(o[0]).all()) for o in diff)
    assert diff[0][0].shape == diff[1][0].shape          # (threshold 1.0: the length is minlen = maxlen)
    assert not torch.equal(diff[0][0], diff[1][0])


# ------------------------------------------------------------------------------------------------------------------------------
# 9. Base size
# ------------------------------------------------------------------------------------------------------------------------------
def _base(cuda, dtype, seed=4246):
    from tests.test_cfg3_shape_gpu import build
    args, task, model = build(cuda, dtype, seed=seed)
    return args, task, model.eval()


def _ragged_texts(vocab, lens, seed=21):
    g = torch.Generator().manual_seed(seed)
    toks = torch.full((len(lens), max(lens)), 1, dtype=torch.long)
    for b, n in enumerate(lens):
        toks[b, :n - 1] = torch.randint(4, vocab - 2, (n - 1,), generator=g)
        toks[b, n - 1] = 2
    spk = torch.randn(len(lens), 512, generator=g)
    return toks, spk


@pytest.mark.parametrize("threshold,stop_bias", [(2.0, 0.0), (None, -0.35)])
def test_base_size_rows_match_oracle(cuda, threshold, stop_bias):
    from oracle import speecht5_oracle as O
    args, task, model = _base(cuda, torch.float32)
    with torch.no_grad():
        model.speech_decoder_postnet.prob_out.bias.fill_(stop_bias)
    lens = [100, 80, 60]
    toks, spk = _ragged_texts(len(task.dicts["text"]), lens)
    kw = {} if threshold is None else {"threshold": threshold}
    out = model.generate_speech_batch(src_tokens=toks.to(cuda), spkembs=spk.to(cuda), **kw)
    sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    cfg = SimpleNamespace(**vars(args))
    for b, n in enumerate(lens):
        if threshold is None:
            single = model.generate_speech(src_tokens=toks[b:b + 1, :n].to(cuda), spkembs=spk[b:b + 1].to(cuda))
            _assert_margin(single[1], 0.5, f"Base row {b}")
        with torch.no_grad():
            ref = O.generate_speech(sd, cfg, toks[b:b + 1, :n], spk[b:b + 1], **kw)
        print(f"Base row {b}: {out[b][0].shape[0] // 2} steps (oracle {ref.shape[0] // 2})")
        assert out[b][0].shape == ref.shape, (b, out[b][0].shape, ref.shape)
        if threshold is not None:
            assert out[b][0].shape[0] == 2 * n
        close(out[b][0], ref, 1e-3, what=f"Base row {b} vs the oracle")


def test_base_size_bf16_batch_of_32_tracks_fp32(cuda):
    lens = [100 - 2 * b for b in range(32)]
    _, task, model = _base(cuda, torch.float32)
    toks, spk = _ragged_texts(len(task.dicts["text"]), lens, seed=5)
    ref = model.generate_speech_batch(src_tokens=toks.to(cuda), spkembs=spk.to(cuda), threshold=2.0, need_attn=False)
    del model
    _, _, model = _base(cuda, torch.bfloat16)
    got = model.generate_speech_batch(src_tokens=toks.to(cuda), spkembs=spk.to(cuda), threshold=2.0, need_attn=False)
    worst = 1.0
    for b, (g, f) in enumerate(zip(got, ref)):
        assert g[0].shape == f[0].shape == (2 * lens[b], 80)
        cos = float(torch.nn.functional.cosine_similarity(g[0].double().flatten(), f[0].double().flatten(), dim=0))
        worst = min(worst, cos)
        assert cos >= 0.999, (b, cos)
    print(f"bf16 vs fp32 at B = 32: worst mel cosine {worst:.6f}")


# ------------------------------------------------------------------------------------------------------------------------------
# 10. task methods
# ------------------------------------------------------------------------------------------------------------------------------
def test_task_generate_speech_methods(cuda, golden):
    from speecht5_amd.collate import TextToSpeechCollater
    from speecht5_amd.task import SpeechT5Task
    model, args = _tiny(cuda)
    task = SpeechT5Task.synthetic(args)
    n = golden.lens[0]
    ni = {"src_tokens": golden.toks[:1, :n].to(cuda), "spkembs": golden.spk[:1].to(cuda), "src_lengths": torch.tensor([n], device=cuda),
          "prev_output_tokens": torch.zeros(1, 4, 80, device=cuda), "task_name": "t2s"}
    got = task.generate_speech([model], ni)
    want = model.generate_speech(src_tokens=ni["src_tokens"], spkembs=ni["spkembs"])
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    g = torch.Generator().manual_seed(9)
    samples = [{"id": b, "audio_name": f"u{b}", "source": [golden.toks[b, :golden.lens[b]].to(cuda)],
                "target": torch.randn(6 + 2 * b, 80, generator=g).to(cuda), "spkembs": golden.spk[b].to(cuda)} for b in range(3)]
    batch = TextToSpeechCollater(cuda, pad_idx=1, reduction_factor=args.reduction_factor).collater(samples)
    assert "prev_output_tokens" in batch["net_input"] and "task_name" in batch["net_input"]
    got = task.generate_speech_batch([model], batch["net_input"])
    want = model.generate_speech_batch(src_tokens=batch["net_input"]["src_tokens"], spkembs=batch["net_input"]["spkembs"])
    assert torch.equal(batch["net_input"]["src_tokens"].cpu(), golden.toks)
    for a, b in zip(got, want):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
