"""Device-stepped and graph-replayed TTS decode on the HIP kernels: csrc/decode_gemm.hip (st5_gemm_skinny), the device-step entries
of csrc/lm_decode.hip / csrc/tts_decode.hip, and generate_speech_batch / synthesize_batch with decode="device" / "graph".

 3. skinny GEMM against the fp64 restatement, yardstick st5_gemm;   3b. its dropout epilogue;   4. row independence bit for bit;
 5. device-side slot write between guards;   6. argument checks;   7. device-step attention / record column / step tail bit-equal
 to the host-step forms;   8. "graph" == "device" bit for bit;   9. the new modes against "eager" and the CPU oracle (tiny and Base);
 10. bf16 at Base, B = 32;   11. row permutation and batch composition;   12. B = 40 and B = 1;   13. synthesize_batch."""
from argparse import Namespace
from types import SimpleNamespace

import pytest
import torch

from tests import tts_graph_reference as R
from tests.test_tts_batch_gpu import _assert_margin, _base, _pick_stop_shift, _ragged_texts, _singles, golden  # noqa: F401
from tests.util import Task, build_tiny, close, load_golden

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


def _rounded(t, dtype):
    return t.to(dtype).float()


def _problem(N, K, M, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * N + K + 1000 * M)
    x = _rounded(torch.randn(M, K, generator=g), dtype)
    w = _rounded(torch.randn(N, K, generator=g) / K ** 0.5, dtype)
    b = torch.randn(N, generator=g)
    res = _rounded(torch.randn(M, N, generator=g), dtype)
    return x, w, b, res


def _skinny(Fn, x, ws, bs, dtype, cuda, **epi):
    res = epi.pop("residual", None)
    W = torch.cat(ws, 0).to(cuda).to(dtype).contiguous()
    b = torch.cat(bs, 0).to(cuda).contiguous() if bs is not None else None
    return Fn.linear_skinny(x.to(cuda).to(dtype), W, b, residual=res.to(cuda).to(dtype) if res is not None else None, **epi)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. accuracy against fp64, yardstick st5_gemm
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,K", R.BASE_SHAPES + R.TINY_SHAPES + R.LM_SHAPES)
def test_skinny_gemm_against_fp64_with_st5_gemm_as_yardstick(cuda, N, K, dtype):
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(dtype)
    for M in (1, 3, 8, 31, 32):
        x, w, b, res = _problem(N, K, M, dtype)
        h = (N // 2 + 7) // 8 * 8
        cases = [("bias", [w], [b], R.ACT_NONE, None, False), ("relu", [w], [b], R.ACT_RELU, None, False),
                 ("ffn-act", [w], [b], R.ACT_GELU, None, False), ("residual", [w], [b], R.ACT_NONE, res, False),
                 ("stacked", [w[:h], w[h:]], [b[:h], b[h:]], R.ACT_NONE, None, False),
                 ("stacked-fp32-out", [w[:h], w[h:]], [b[:h], b[h:]], R.ACT_NONE, None, True)]
        for name, ws, bs, act, r_, f32 in cases:
            ref = R.skinny_gemm(x, ws, bs, act, r_)
            got = _skinny(Fn, x, ws, bs, dtype, cuda, act=act, residual=r_, out_f32=f32)
            assert got.dtype == (torch.float32 if f32 else dtype)
            with torch.no_grad():
                if r_ is not None and N % 8:
                    # st5_gemm adds a residual only at 8-aligned widths: its form at this width is the plain launch and an add in the
                    # compute dtype behind it
                    old = Fn.linear(x.to(cuda).to(dtype), [t.to(cuda) for t in ws], [t.to(cuda) for t in bs], act=act) + r_.to(cuda).to(dtype)
                else:
                    old = Fn.linear(x.to(cuda).to(dtype), [t.to(cuda) for t in ws], [t.to(cuda) for t in bs], act=act,
                                    residual=r_.to(cuda).to(dtype) if r_ is not None else None)   # (bf16 output: the yardstick of fp32-out too)
            e_new = float((got.double().cpu() - ref).abs().max())
            e_old = float((old.double().cpu() - ref).abs().max())
            floor = R.ulp_at_scale(ref, torch.float32 if f32 else dtype)
            print(f"({N}, {K}) M={M} {name}: skinny {e_new:.3e}  st5_gemm {e_old:.3e}  floor {floor:.3e}")
            assert e_new <= 1.5 * e_old + floor, (N, K, M, name, e_new, e_old, floor)
        Fn.weight_cache.clear()


# ------------------------------------------------------------------------------------------------------------------------------
# 3b. dropout epilogue
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dropout_epilogue(cuda, dtype):
    from speecht5_amd import functional as Fn
    M, N, K = 32, 256, 80
    g = torch.Generator().manual_seed(3)
    x = torch.rand(M, K, generator=g) + 0.1
    x[1] = x[0]                                                   # two identical rows
    w = torch.rand(N, K, generator=g) / K
    b = torch.rand(N, generator=g)
    run = lambda **kw: _skinny(Fn, x, [w], [b], dtype, cuda, act=R.ACT_RELU, **kw)   # noqa: E731
    plain = _skinny(Fn, x, [w], [b], dtype, cuda, act=R.ACT_RELU)
    assert torch.equal(run(dropout_p=0.0, seed=5), plain)
    assert bool((plain > 0).all())
    a = run(dropout_p=0.5, seed=1234)
    kept = a != 0
    assert torch.equal(a[kept].float(), 2 * plain[kept].float()), "a kept element is exactly twice its p = 0 value"
    frac = float(kept.float().mean())
    print(f"kept fraction {frac:.4f}")
    assert abs(frac - 0.5) <= 0.0221
    assert torch.equal(a, run(dropout_p=0.5, seed=1234))
    assert not torch.equal(a, run(dropout_p=0.5, seed=1235))
    assert not torch.equal(a[0], a[1]), "two identical rows must draw different masks"
    slot = torch.tensor([1234], dtype=torch.int64, device=cuda)     # the same seed through a seed slot
    assert torch.equal(a, run(dropout_p=0.5, seed=(1 << 63) | slot.data_ptr()))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. row independence
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,K", [(768, 768), (162, 768), (768, 3072), (256, 80), (128, 192)])
def test_rows_are_independent_bit_for_bit(cuda, N, K, dtype):
    from speecht5_amd import functional as Fn
    for M in (32, 5):
        x, w, b, res = _problem(N, K, M, dtype, seed=11)
        h = (N // 2 + 7) // 8 * 8
        for ws, bs, r_ in (([w], [b], None), ([w[:h], w[h:]], [b[:h], b[h:]], None), ([w], [b], res)):
            full = _skinny(Fn, x, ws, bs, dtype, cuda, residual=r_)
            for m in range(M):
                xn = torch.full_like(x, float("nan"))
                xn[m] = x[m]
                rn = None
                if r_ is not None:
                    rn = torch.full_like(r_, float("nan"))
                    rn[m] = r_[m]
                among_nan = _skinny(Fn, xn, ws, bs, dtype, cuda, residual=rn)
                alone = _skinny(Fn, x[m:m + 1], ws, bs, dtype, cuda, residual=r_[m:m + 1] if r_ is not None else None)
                assert torch.equal(full[m], alone[0]), (M, m)
                assert torch.equal(full[m], among_nan[m]), (M, m)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. slot write, 6. argument checks
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_slot_write_follows_the_device_counter_and_stays_inside(cuda, dtype):
    from speecht5_amd import functional as Fn
    B, cap, C = 5, 6, 128
    x, w, b, _ = _problem(2 * C, C, B, dtype, seed=2)
    fixed = _skinny(Fn, x, [w], [b], dtype, cuda)
    n, guard = B * cap * 2 * C, 4096
    for step, slot in ((0, 0), (1, 1), (cap - 1, cap - 1), (cap, cap - 1), (-1, 0)):
        whole = torch.full((guard + n + guard,), -7.0, dtype=dtype, device=cuda)   # guards and buffer: ONE allocation
        buf = whole[guard:guard + n].view(B, cap, 2 * C)
        counter = torch.tensor([step], dtype=torch.int32, device=cuda)
        _skinny(Fn, x, [w], [b], dtype, cuda, out=buf, step=counter, step_stride=2 * C, step_cap=cap, out_ld=cap * 2 * C)
        torch.cuda.synchronize()
        assert bool((whole[:guard] == -7.0).all()) and bool((whole[guard + n:] == -7.0).all()), f"step {step}: a guard was written"
        assert torch.equal(buf[:, slot], fixed), f"step {step}"
        rest = torch.cat([buf[:, :slot], buf[:, slot + 1:]], dim=1)
        assert bool((rest == -7.0).all()), f"step {step}: another slot was written"
        assert int(counter) == step


def test_argument_checks(cuda):
    from speecht5_amd import functional as Fn
    from speecht5_amd import hip
    L = hip.lib()
    x = torch.zeros(40, 72, device=cuda)
    w = torch.zeros(64, 72, device=cuda)
    out = torch.zeros(40, 64, device=cuda)

    def call(M, x_ld, K=64, act=0):
        return L.st5_gemm_skinny(x.data_ptr(), x_ld, w.data_ptr(), 72, 0, 0, 0, out.data_ptr(), 64, M, 64, K, act, 0.0, 0, 0, 0, 0, 0, 0, 0,
                                 hip.F32, hip.stream())
    assert call(32, 72) == 0
    assert call(33, 72) == 1          # ST5_ERR_ARG
    assert call(0, 72) == 1
    assert call(4, 72, act=4) == 1    # an epilogue the kernel does not have
    assert call(4, 71) == 2           # ST5_ERR_ALIGN: odd leading dimension
    assert L.st5_gemm_skinny(x.data_ptr() + 4, 72, w.data_ptr(), 72, 0, 0, 0, out.data_ptr(), 64, 4, 64, 64, 0, 0.0, 0, 0, 0, 0, 0, 0, 0,
                             hip.F32, hip.stream()) == 2
    torch.cuda.synchronize()
    big = Fn.linear_skinny(torch.ones(40, 72, device=cuda), torch.ones(64, 72, device=cuda))   # the wrapper chunks the rows
    assert bool((big == 72.0).all())


# ------------------------------------------------------------------------------------------------------------------------------
# 7. device-step forms bit-equal to the host-step forms
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,H,hd", [(3, 12, 64), (32, 12, 64), (3, 16, 80)])
def test_device_t_self_attention_is_bit_equal(cuda, B, H, hd, dtype):
    from speecht5_amd import functional as Fn
    cap, C = 1000, H * hd
    g = torch.Generator().manual_seed(B + hd)
    q = torch.randn(B, C, generator=g).to(dtype).to(cuda)
    kv = torch.randn(B, cap, 2 * C, generator=g).to(dtype).to(cuda)
    anc = torch.arange(B, dtype=torch.int32, device=cuda).unsqueeze(1).expand(B, cap).contiguous()
    ws = Fn.lm_decode_attn_ws(B, cap, H, hd, cuda)
    ctx = torch.empty(B, C, dtype=dtype, device=cuda)
    for t in (1, 63, 64, 65, 128, 129, 500, cap):
        want = Fn.lm_decode_attn(q, kv, anc, t, H, hd)
        ctx.fill_(float("nan"))
        Fn.lm_decode_attn_dev(q, kv, anc, torch.tensor([t - 1], dtype=torch.int32, device=cuda), 1, cap, H, hd, ctx, ws)
        assert torch.equal(ctx, want), f"t = {t}"
        ctx.fill_(float("nan"))
        Fn.lm_decode_attn_dev(q, kv, anc, torch.tensor([t], dtype=torch.int32, device=cuda), 0, cap, H, hd, ctx, ws)
        assert torch.equal(ctx, want), f"t = {t} (t_add 0)"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,S", [(3, 40), (32, 100), (3, 499)])
def test_device_step_cross_attention_record_is_bit_equal(cuda, B, S, dtype):
    from speecht5_amd import functional as Fn
    H, hd, cap = 12, 64, 5
    C = H * hd
    g = torch.Generator().manual_seed(B + S)
    q = torch.randn(B, C, generator=g).to(dtype).to(cuda)
    kv = torch.randn(B * S, 2 * C, generator=g).to(dtype).to(cuda)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    kpm = (torch.arange(S)[None, :] >= lens[:, None]).to(torch.uint8).to(cuda)
    ws = Fn.decode_cross_attn_ws(B, S, H, hd, cuda)
    for col in (0, 3, cap - 1):
        rec = torch.full((B, H, cap, S), 7.0, device=cuda)
        want_ctx = Fn.decode_cross_attn(q, kv, 0, S, H, hd, kpm=kpm, probs=(rec[:, :, col], rec.stride(0), rec.stride(1)), ws=ws)
        rec2 = torch.full((B, H, cap, S), 7.0, device=cuda)
        ctx = torch.empty(B, C, dtype=dtype, device=cuda)
        Fn.decode_cross_attn_step(q, kv, 0, S, H, hd, ctx, torch.tensor([col], dtype=torch.int32, device=cuda), cap, kpm=kpm, rec=rec2, ws=ws)
        assert torch.equal(ctx, want_ctx) and torch.equal(rec2, rec), f"column {col}"
        ctx2 = torch.empty(B, C, dtype=dtype, device=cuda)
        Fn.decode_cross_attn_step(q, kv, 0, S, H, hd, ctx2, torch.tensor([col], dtype=torch.int32, device=cuda), cap, kpm=kpm, ws=ws)
        assert torch.equal(ctx2, want_ctx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_device_step_tail_is_bit_equal_and_stops_at_the_cap(cuda, dtype):
    from speecht5_amd import functional as Fn
    B, r, odim, cap, thr = 7, 2, 80, 5, 0.5
    g = torch.Generator().manual_seed(7)
    y = torch.randn(B, r * odim + r + 3, generator=g).to(cuda)
    minlen = torch.tensor([0, 4, 0, 0, 0, 0, 3], dtype=torch.int32, device=cuda)
    maxlen = torch.tensor([9, 9, 3, 9, 9, 9, 2], dtype=torch.int32, device=cuda)

    def state():
        return (torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.int32, device=cuda), torch.tensor([0, 0, 0, 2, 0, 0, 0], dtype=torch.int32, device=cuda),
                torch.full((B, cap * r, odim), -5.0, device=cuda), torch.full((B, cap * r), -5.0, device=cuda),
                torch.full((B, odim), -5.0, device=cuda).to(dtype), torch.full((1,), -1, dtype=torch.int32, device=cuda))
    table = torch.arange(cap * 2, dtype=torch.int64, device=cuda).view(cap, 2) + 100
    for idx in (1, 3, cap):
        a, b = state(), state()
        Fn.tts_step_tail(y, r, odim, minlen, maxlen, a[0], a[1], idx, thr, a[2], a[3], a[4], a[5])
        counter = torch.tensor([idx - 1], dtype=torch.int32, device=cuda)
        slots = torch.zeros(2, dtype=torch.int64, device=cuda)
        Fn.tts_step_tail_dev(y, r, odim, minlen, maxlen, b[0], b[1], counter, thr, b[2], b[3], b[4], b[5], table, slots)
        for u, v in zip(a, b):
            assert torch.equal(u, v), idx
        assert int(counter) == idx
        assert slots.tolist() == (table[idx].tolist() if idx < cap else [0, 0]), "the next step's seeds are moved into the slots"
    for past in (cap, cap + 3, -2):
        a, b = state(), state()
        counter = torch.tensor([past], dtype=torch.int32, device=cuda)
        Fn.tts_step_tail_dev(y, r, odim, minlen, maxlen, b[0], b[1], counter, thr, b[2], b[3], b[4], b[5])
        for u, v in zip(a, b):
            assert torch.equal(u, v), f"counter {past}: something was written"
        assert int(counter) == past


# ------------------------------------------------------------------------------------------------------------------------------
# 8. "graph" == "device" bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
def _tiny(cuda, dtype=torch.float32, pre_ln=False):
    if not pre_ln:
        model, args = build_tiny(cuda, dtype)
        return model.eval(), args
    from speecht5_amd import functional as Fn
    from speecht5_amd.speecht5 import T5TransformerModel
    m, _ = load_golden(None)
    args = Namespace(**dict(m["args"], decoder_normalize_before=True))
    Fn.set_compute_dtype(dtype)
    torch.manual_seed(3)
    model = T5TransformerModel.build_model(args, Task())
    torch.nn.Module.load_state_dict(model, m["state_dict"], strict=False)
    with torch.no_grad():
        model.decoder.layer_norm.weight.uniform_(0.5, 1.5)
        model.decoder.layer_norm.bias.uniform_(-0.1, 0.1)
    return model.to(cuda).eval(), args


def _equal_rows(a, b):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        for k, (s, t) in enumerate(zip(u, v)):
            assert (s is None) == (t is None), (i, k)
            assert s is None or torch.equal(s, t), (i, k)


def _speech_rows(cuda):
    g = torch.Generator().manual_seed(55)
    n = [16000, 40000, 27200]
    src = torch.zeros(3, max(n))
    pad = torch.ones(3, max(n), dtype=torch.bool)
    for b, m in enumerate(n):
        src[b, :m] = torch.randn(m, generator=g) * 0.1
        pad[b, :m] = False
    return src.to(cuda), pad.to(cuda)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pre_ln", [False, True], ids=["post-ln", "pre-ln"])
def test_graph_equals_device_bit_for_bit(cuda, golden, pre_ln, dtype):
    from speecht5_amd import functional as Fn
    model, _ = _tiny(cuda, dtype, pre_ln)
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    src, pad = _speech_rows(cuda)
    tac = model.speech_decoder_prenet.decoder_prenet[0][0]
    inputs = [dict(src_tokens=toks, spkembs=spk), dict(src_tokens=toks, spkembs=spk, need_attn=False),
              dict(source=src, padding_mask=pad, spkembs=spk)]
    for p_drop in (0.0, 0.5):
        tac.dropout_rate = p_drop
        try:
            for kw in inputs:
                Fn.manual_seed(77)
                dev = model.generate_speech_batch(decode="device", **kw)
                assert model.tts_decode_mode == "device" and model.tts_graph_replays == 0 and model.tts_device_steps > 0
                polls = model.tts_polls
                Fn.manual_seed(77)
                gr = model.generate_speech_batch(decode="graph", **kw)
                assert model.tts_decode_mode == "graph" and model.tts_graph_replays > 0
                assert model.tts_polls == polls
                _equal_rows(gr, dev)
                assert all(bool(torch.isfinite(o[0]).all()) for o in gr)
        finally:
            tac.dropout_rate = 0.0
    model.generate_speech_batch(src_tokens=toks, spkembs=spk)
    assert model.tts_decode_mode == "eager" and model.tts_graph_replays == 0


def test_explicit_modes_refuse_a_training_model_and_unknown_names(cuda, golden):
    model, _ = _tiny(cuda)
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    with pytest.raises(ValueError, match="decode"):
        model.generate_speech_batch(src_tokens=toks, spkembs=spk, decode="fast")
    model.train()
    try:
        for mode in ("device", "graph"):
            with pytest.raises(RuntimeError, match="training mode"):
                model.generate_speech_batch(src_tokens=toks, spkembs=spk, decode=mode)
    finally:
        model.eval()


# ------------------------------------------------------------------------------------------------------------------------------
# 9. the new modes against "eager" and the CPU oracle
# ------------------------------------------------------------------------------------------------------------------------------
def _err(a, ref):
    """The `close` measure: largest absolute difference over the reference's largest magnitude."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)


def _check_against_eager_and_oracle(tag, new, eager, oracle_mels, r, thr):
    assert len(new) == len(eager) == len(oracle_mels)
    for b, (g, e, ref) in enumerate(zip(new, eager, oracle_mels)):
        _assert_margin(e[1], thr, f"{tag} row {b} (eager)")
        _assert_margin(g[1], thr, f"{tag} row {b}")
        assert g[0].shape == e[0].shape == ref.shape, (tag, b, g[0].shape, e[0].shape, ref.shape)
        close(g[0], ref, 1e-3, what=f"{tag} row {b} vs the oracle")
        e_eager, e_new = _err(e[0], ref), _err(g[0], ref)
        d = [_err(g[k], e[k]) for k in range(3) if g[k] is not None and e[k] is not None]
        line = (f"{tag} row {b}: {g[0].shape[0] // r} steps; vs oracle: eager {e_eager:.3e}, new {e_new:.3e}; new vs eager (mel, probs, attn): "
                + ", ".join(f"{v:.3e}" for v in d))
        print(line)
        assert e_new <= max(2 * e_eager, 1e-5), (tag, b, e_new, e_eager)


def test_tiny_new_modes_match_eager_and_oracle_with_data_dependent_stops(cuda, golden):
    from oracle import speecht5_oracle as O
    from speecht5_amd import functional as Fn
    model, args = _tiny(cuda)
    r = args.reduction_factor
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    maxlen = [int(n * 20.0 / r) for n in golden.lens]
    shift, stops = _pick_stop_shift(_singles(model, toks, spk, golden.lens), r, maxlen)
    with torch.no_grad():
        model.speech_decoder_postnet.prob_out.bias.add_(shift)
    Fn.weight_cache.clear()
    sd = {k: v.clone() for k, v in golden.sd.items()}
    sd["speech_decoder_postnet.prob_out.bias"] = sd["speech_decoder_postnet.prob_out.bias"] + shift
    with torch.no_grad():
        refs = [O.generate_speech(sd, golden.cfg, golden.toks[b:b + 1, :golden.lens[b]], golden.spk[b:b + 1]) for b in range(3)]
    eager = model.generate_speech_batch(src_tokens=toks, spkembs=spk)
    for mode in ("device", "graph"):
        out = model.generate_speech_batch(src_tokens=toks, spkembs=spk, decode=mode)
        lens = [o[0].shape[0] // r for o in out]
        print(f"{mode}: stop-logit shift {shift:+.4f}: steps {lens} (predicted {stops}, maxlen {maxlen})")
        assert lens == stops == [o[0].shape[0] // r for o in eager]
        assert len(set(lens)) >= 2
        assert any(n % model.TTS_POLL_STEPS != 0 and n < ml for n, ml in zip(lens, maxlen)), "no row stops between two polls"
        _check_against_eager_and_oracle(f"tiny {mode}", out, eager, refs, r, 0.5)


@pytest.mark.parametrize("threshold,stop_bias", [(2.0, 0.0), (None, -0.35)])
def test_base_size_graph_matches_eager_and_oracle(cuda, threshold, stop_bias):
    from oracle import speecht5_oracle as O
    args, task, model = _base(cuda, torch.float32)
    with torch.no_grad():
        model.speech_decoder_postnet.prob_out.bias.fill_(stop_bias)
    lens = [100, 80, 60]
    toks, spk = _ragged_texts(len(task.dicts["text"]), lens)
    kw = {} if threshold is None else {"threshold": threshold}
    eager = model.generate_speech_batch(src_tokens=toks.to(cuda), spkembs=spk.to(cuda), **kw)
    out = model.generate_speech_batch(src_tokens=toks.to(cuda), spkembs=spk.to(cuda), decode="graph", **kw)
    assert model.tts_decode_mode == "graph" and model.tts_graph_replays > 0
    sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    cfg = SimpleNamespace(**vars(args))
    with torch.no_grad():
        refs = [O.generate_speech(sd, cfg, toks[b:b + 1, :n], spk[b:b + 1], **kw) for b, n in enumerate(lens)]
    _check_against_eager_and_oracle(f"Base thr={threshold}", out, eager, refs, args.reduction_factor, 0.5 if threshold is None else threshold)


# ------------------------------------------------------------------------------------------------------------------------------
# 10. bf16 at Base, B = 32
# ------------------------------------------------------------------------------------------------------------------------------
def test_base_size_bf16_graph_batch_of_32_tracks_fp32(cuda):
    lens = [100 - 2 * b for b in range(32)]
    _, task, model = _base(cuda, torch.float32)
    toks, spk = _ragged_texts(len(task.dicts["text"]), lens, seed=5)
    ref = model.generate_speech_batch(src_tokens=toks.to(cuda), spkembs=spk.to(cuda), threshold=2.0, need_attn=False)
    del model
    _, _, model = _base(cuda, torch.bfloat16)
    old = model.generate_speech_batch(src_tokens=toks.to(cuda), spkembs=spk.to(cuda), threshold=2.0, need_attn=False)
    got = model.generate_speech_batch(src_tokens=toks.to(cuda), spkembs=spk.to(cuda), threshold=2.0, need_attn=False, decode="graph")
    assert model.tts_decode_mode == "graph" and model.tts_graph_replays > 0
    cos = lambda a, b: float(torch.nn.functional.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))   # noqa: E731
    worst, worst_old = 1.0, 1.0
    for b, (g, o, f) in enumerate(zip(got, old, ref)):
        assert g[0].shape == f[0].shape == (2 * lens[b], 80)
        worst, worst_old = min(worst, cos(g[0], f[0])), min(worst_old, cos(o[0], f[0]))
    print(f"bf16 vs eager fp32 at B = 32: worst mel cosine graph {worst:.6f}, eager bf16 {worst_old:.6f}")
    assert worst >= 0.999, worst


# ------------------------------------------------------------------------------------------------------------------------------
# 11. row permutation and batch composition
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_graph_rows_are_bit_identical_under_permutation_and_composition(cuda, golden, dtype):
    model, _ = _tiny(cuda, dtype)
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    perm = [2, 0, 1]
    out = model.generate_speech_batch(src_tokens=toks, spkembs=spk, decode="graph")
    outp = model.generate_speech_batch(src_tokens=toks[perm], spkembs=spk[perm], decode="graph")
    for i, b in enumerate(perm):
        for k in range(3):
            assert torch.equal(outp[i][k], out[b][k]), (i, b, k)
    other = toks.clone()
    n = golden.lens[0]
    for b in (1, 2):                    # every other row's text replaced (same lengths, so the padded batch keeps its shape)
        m = golden.lens[b]
        other[b, :m - 1] = toks[0, :n - 1].flip(0).repeat(4)[:m - 1]
    assert not torch.equal(other, toks)
    out2 = model.generate_speech_batch(src_tokens=other, spkembs=spk, decode="graph")
    for k in range(3):
        assert torch.equal(out2[0][k], out[0][k]), k


# ------------------------------------------------------------------------------------------------------------------------------
# 12. B = 40 and B = 1
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [40, 1])
def test_other_batch_sizes_in_both_modes(cuda, golden, B):
    from oracle import speecht5_oracle as O
    model, args = _tiny(cuda)
    r = args.reduction_factor
    rows = [(b % 3, max(2, golden.lens[b % 3] - (b // 3) % 3)) for b in range(B)]        # golden rows repeated, lengths varied by truncation
    width = max(n for _, n in rows)
    toks = torch.full((B, width), 1, dtype=torch.long)
    for i, (b, n) in enumerate(rows):
        toks[i, :n - 1] = golden.toks[b, :n - 1]
        toks[i, n - 1] = 2
    spk = golden.spk[[b for b, _ in rows]]
    cache = {}
    refs = []
    with torch.no_grad():
        for i, key in enumerate(rows):
            if key not in cache:
                cache[key] = O.generate_speech(golden.sd, golden.cfg, toks[i:i + 1, :key[1]], spk[i:i + 1])
            refs.append(cache[key])
    eager = model.generate_speech_batch(src_tokens=toks.to(cuda), spkembs=spk.to(cuda))
    for mode in ("device", "graph"):
        out = model.generate_speech_batch(src_tokens=toks.to(cuda), spkembs=spk.to(cuda), decode=mode)
        assert model.tts_decode_mode == mode and (model.tts_graph_replays > 0) == (mode == "graph")
        _check_against_eager_and_oracle(f"B={B} {mode}", out, eager, refs, r, 0.5)


# ------------------------------------------------------------------------------------------------------------------------------
# 13. synthesize_batch
# ------------------------------------------------------------------------------------------------------------------------------
def test_synthesize_batch_graph(cuda, golden):
    from oracle import speecht5_oracle as O
    from tests.test_tts_wave_gpu import _vocoder
    model, args = _tiny(cuda)
    vocoder, _, _ = _vocoder(cuda, "tiny", torch.float32)
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    eager = model.synthesize_batch(src_tokens=toks, spkembs=spk, vocoder=vocoder, need_attn=True)
    out = model.synthesize_batch(src_tokens=toks, spkembs=spk, vocoder=vocoder, need_attn=True, decode="graph")
    assert model.tts_decode_mode == "graph" and model.tts_graph_replays > 0
    with torch.no_grad():
        refs = [O.generate_speech(golden.sd, golden.cfg, golden.toks[b:b + 1, :golden.lens[b]], golden.spk[b:b + 1]) for b in range(3)]
    assert [o[1].shape for o in out] == [e[1].shape for e in eager]
    assert [o[0].shape for o in out] == [e[0].shape for e in eager]
    _check_against_eager_and_oracle("synthesize graph", [o[1:] for o in out], [e[1:] for e in eager], refs, args.reduction_factor, 0.5)
    for b, o in enumerate(out):
        close(o[0], vocoder(o[1]).reshape(-1), 1e-5, what=f"row {b} waveform against vocoder.forward on the returned mel")


def test_task_methods_pass_decode_through(cuda, golden):
    from speecht5_amd.collate import TextToSpeechCollater
    from speecht5_amd.task import SpeechT5Task
    model, args = _tiny(cuda)
    task = SpeechT5Task.synthetic(args)
    g = torch.Generator().manual_seed(9)
    samples = [{"id": b, "audio_name": f"u{b}", "source": [golden.toks[b, :golden.lens[b]].to(cuda)],
                "target": torch.randn(6 + 2 * b, 80, generator=g).to(cuda), "spkembs": golden.spk[b].to(cuda)} for b in range(3)]
    batch = TextToSpeechCollater(cuda, pad_idx=1, reduction_factor=args.reduction_factor).collater(samples)
    want = model.generate_speech_batch(src_tokens=batch["net_input"]["src_tokens"], spkembs=batch["net_input"]["spkembs"], decode="graph")
    got = task.generate_speech_batch([model], batch["net_input"], decode="graph")
    assert model.tts_decode_mode == "graph" and model.tts_graph_replays > 0
    _equal_rows(got, want)
    got = task.synthesize_batch([model], batch["net_input"], decode="device")
    assert model.tts_decode_mode == "device" and model.tts_device_steps > 0
    for a, b in zip(got, want):
        assert a[0] is None and torch.equal(a[2], b[1])
    with pytest.raises(ValueError, match="decode"):
        task.generate_speech_batch([model], batch["net_input"], decode="fast")


def test_graph_mode_keeps_one_stream_per_model(cuda, golden):
    model, _ = _tiny(cuda)
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    from speecht5_amd.tts_graph import decode_stream
    model.generate_speech_batch(src_tokens=toks, spkembs=spk, decode="graph")
    first = decode_stream(model, cuda)
    model.generate_speech_batch(src_tokens=toks, spkembs=spk, decode="graph")
    assert decode_stream(model, cuda) == first and len(model._tts_graph_streams) == 1
    own = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(own):
        assert decode_stream(model, cuda) == own            # a caller's own (capturable) stream is used as it is
        out = model.generate_speech_batch(src_tokens=toks, spkembs=spk, decode="graph")
    own.synchronize()
    _equal_rows(out, model.generate_speech_batch(src_tokens=toks, spkembs=spk, decode="graph"))
