"""The LayerDrop layer gate: every native launch of a gated transformer layer carries the layer's `keep` float and exits
at once when the layer is dropped.  Kernel level, through the C ABI: gate NULL == keep 1 == the ungated call, byte for byte; keep 0
leaves dead outputs untouched (NaN pre-fill, bytes compared) and gives live outputs exact zeros / unchanged accumulators.  Model
level: the exit form == the select-only form (ST5_LAYER_EXIT=0), byte for byte, also with every output of a gated launch allocated
NaN-filled; replayed side-by-side updates == eager in-turn ones."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from speecht5_amd import functional as Fn
from speecht5_amd import hip
from tests.util import Task, load_golden, to_dev

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _nan(*shape, dtype=BF, device=None):
    return torch.full(shape, NAN, dtype=dtype, device=device)


def _keep(cuda, v):
    return None if v is None else torch.tensor([float(v)], device=cuda)


class _gate:
    """hip.gemm / Fn launches inside carry `keep` (a one-float device tensor or None) as the ambient layer gate."""

    def __init__(self, keep):
        self.keep = keep

    def __enter__(self):
        self.prev = Fn._lgate_set(self.keep)

    def __exit__(self, *exc):
        Fn._lgate_set(self.prev)


# ------------------------------------------------------------------------------------------------- 1. NT GEMM
_NT_CASES = [(256, 256, 128, 0), (130, 72, 64, 0), (256, 256, 128, 3), (256, 256, 128, 5)]


@pytest.mark.parametrize("M,N,K,tile", _NT_CASES)
@pytest.mark.parametrize("epi", ["plain", "bias_gelu_pre", "bias_drop_res", "dact"])
def test_nt_gemm_gate(cuda, M, N, K, tile, epi):
    torch.manual_seed(M + N + tile)
    A = (torch.randn(M, K) * 0.5).to(BF).to(cuda)
    B = (torch.randn(N, K) * 0.5).to(BF).to(cuda)
    bias = torch.randn(N, device=cuda)
    R = torch.randn(M, N).to(BF).to(cuda)
    P = torch.randn(M, N).to(BF).to(cuda)

    def run(keep):
        C, Cpre = _nan(M, N, device=cuda), _nan(M, N, device=cuda)
        kw = {}
        if epi == "bias_gelu_pre":
            kw = dict(bias=bias, act=hip.ACT_GELU, Cpre=hip.operand(Cpre, N))
        elif epi == "bias_drop_res":
            kw = dict(bias=bias, dropout_p=0.1, seed=1234, R=hip.operand(R, N))
        elif epi == "dact":
            kw = dict(P=hip.operand(P, N), act=hip.ACT_GELU, flags=hip.DACT)
        with _gate(keep):
            hip.gemm(hip.operand(A, K), hip.operand(B, K), hip.operand(C, N), M, N, K, hip.BF16, **kw)
        torch.cuda.synchronize()
        return C, Cpre

    hip.check(hip.lib().st5_gemm_set_nt_tile(tile), "nt tile")
    try:
        ref, one, zero = run(None), run(_keep(cuda, 1)), run(_keep(cuda, 0))
    finally:
        hip.check(hip.lib().st5_gemm_set_nt_tile(0), "nt tile")
    assert not torch.isnan(ref[0]).any()
    assert _same_bytes(ref[0], one[0]) and _same_bytes(ref[1], one[1])
    if epi == "bias_gelu_pre":
        assert not torch.isnan(ref[1]).any()
    untouched = _nan(M, N, device=cuda)
    assert _same_bytes(zero[0], untouched) and _same_bytes(zero[1], untouched)


# ------------------------------------------------------------------------------------------------- 2. grouped TN, split-K
_TN = hip.A_KSTRIDED | hip.B_KSTRIDED | hip.OUT_F32


def _tn_problem(cuda, M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(K, M, generator=g) * 0.25).to(BF).to(cuda)      # dY [tokens, M], k-strided
    B = (torch.randn(K, N, generator=g) * 0.25).to(BF).to(cuda)      # X  [tokens, N], k-strided
    C0 = torch.randn(M, N, generator=g).to(cuda)                     # pre-seeded accumulators
    s0 = torch.randn(M, generator=g).to(cuda)
    return A, B, C0, s0


def test_grouped_tn_gate_per_problem(cuda):
    shapes = [(256, 256, 512), (256, 768, 520), (128, 256, 512)]     # two phased 256^2 problems (one launch), one of the 128^2 class
    assert [bool(hip.lib().st5_gemm_tn_group_is_phased(*s)) for s in shapes] == [True, True, False]
    probs = [_tn_problem(cuda, *s, seed=i) for i, s in enumerate(shapes)]

    def run(gates):
        out = [(p[2].clone(), p[3].clone()) for p in probs]
        lst = []
        for (A, B, _, _), (C, asum), (M, N, K), gt in zip(probs, out, shapes, gates):
            lst.append((hip.operand(A, M), hip.operand(B, N), hip.operand(C, N), M, N, K, _TN, 1.0, asum, 0 if gt is None else gt.data_ptr()))
        hip.gemm_tn_group(lst, hip.BF16)
        torch.cuda.synchronize()
        return out

    k1, k0 = _keep(cuda, 1), _keep(cuda, 0)
    ref = run([None, None, None])
    one = run([k1, k1, k1])
    mid = run([k1, k0, None])
    for j in range(3):
        assert not _same_bytes(ref[j][0], probs[j][2]) and not _same_bytes(ref[j][1], probs[j][3])     # the ungated group did accumulate
        assert _same_bytes(ref[j][0], one[j][0]) and _same_bytes(ref[j][1], one[j][1])
    assert _same_bytes(mid[1][0], probs[1][2]) and _same_bytes(mid[1][1], probs[1][3]), "the dropped problem's C / asum changed"
    for j in (0, 2):
        assert _same_bytes(mid[j][0], ref[j][0]) and _same_bytes(mid[j][1], ref[j][1]), "a kept problem differs from the ungated group"
    # the 128^2 class, dropped
    last = run([None, None, k0])
    assert _same_bytes(last[2][0], probs[2][2]) and _same_bytes(last[2][1], probs[2][3])


@pytest.mark.parametrize("deferred", [True, False])
def test_splitk_tn_gate(cuda, deferred):
    M, N, K = 256, 256, 4096
    A, B, C0, s0 = _tn_problem(cuda, M, N, K, seed=7)
    L, st = hip.lib(), hip.stream()

    def run(keep):
        C, asum = C0.clone(), s0.clone()
        hip.check(L.st5_gemm_defer_splitk(1 if deferred else 0, st), "defer")
        try:
            with _gate(keep):
                hip.gemm(hip.operand(A, M), hip.operand(B, N), hip.operand(C, N), M, N, K, hip.BF16, flags=_TN | hip.DEFERRABLE, beta=1.0, asum=asum)
            hip.check(L.st5_gemm_flush_splitk(st), "flush")
        finally:
            hip.check(L.st5_gemm_defer_splitk(0, st), "defer off")
        torch.cuda.synchronize()
        return C, asum

    ref, one, zero = run(None), run(_keep(cuda, 1)), run(_keep(cuda, 0))
    assert not _same_bytes(ref[0], C0)
    assert _same_bytes(ref[0], one[0]) and _same_bytes(ref[1], one[1])
    assert _same_bytes(zero[0], C0) and _same_bytes(zero[1], s0)


# ------------------------------------------------------------------------------------------------- 3. LayerNorm
def _ln_fwd(cuda, X, G, Bt, keep, skip, gate, entry):
    rows, cols = X.shape
    L = hip.lib()
    Y, mean, rstd = _nan(rows, cols, device=cuda), _nan(rows, dtype=torch.float32, device=cuda), _nan(rows, dtype=torch.float32, device=cuda)
    a = (X.data_ptr(), G.data_ptr(), Bt.data_ptr(), Y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, cols, 1e-5)
    if entry == "plain":
        hip.check(L.st5_layernorm_fwd(*a, hip.BF16, hip.stream()), "fwd")
    elif entry == "gated":
        hip.check(L.st5_layernorm_gated_fwd(*a, keep.data_ptr(), skip.data_ptr(), hip.BF16, hip.stream()), "gated fwd")
    else:
        hip.check(L.st5_layernorm_fwd_gate(*a, hip.ptr(keep), hip.ptr(skip), hip.ptr(gate), hip.BF16, hip.stream()), "fwd gate")
    torch.cuda.synchronize()
    return Y, mean, rstd


def test_layernorm_fwd_gate(cuda):
    rows, cols = 9, 768
    torch.manual_seed(3)
    X = (torch.randn(rows, cols) * 2 + 0.5).to(BF).to(cuda)
    SK = torch.randn(rows, cols).to(BF).to(cuda)
    G, Bt = torch.randn(cols).to(cuda), torch.randn(cols).to(cuda)
    k1, k0 = _keep(cuda, 1), _keep(cuda, 0)
    ref = _ln_fwd(cuda, X, G, Bt, None, None, None, "plain")
    for got in (_ln_fwd(cuda, X, G, Bt, None, None, None, "gate"), _ln_fwd(cuda, X, G, Bt, None, None, k1, "gate"),
                _ln_fwd(cuda, X, G, Bt, k1, SK, k1, "gate"), _ln_fwd(cuda, X, G, Bt, k1, SK, None, "gate"), _ln_fwd(cuda, X, G, Bt, k1, SK, None, "gated")):
        assert all(_same_bytes(a, b) for a, b in zip(ref, got))
    assert not torch.isnan(ref[0]).any() and not torch.isnan(ref[1]).any()
    # dropped, plain LayerNorm inside the layer: nothing written
    y, mean, rstd = _ln_fwd(cuda, X, G, Bt, None, None, k0, "gate")
    assert torch.isnan(y).all() and torch.isnan(mean).all() and torch.isnan(rstd).all()
    # dropped, the layer's last LayerNorm: y = skip, x never read (all NaN), statistics not written
    XN = _nan(rows, cols, device=cuda)
    y, mean, rstd = _ln_fwd(cuda, XN, G, Bt, k0, SK, k0, "gate")
    assert _same_bytes(y, SK) and torch.isnan(mean).all() and torch.isnan(rstd).all()
    # ... the same bytes as the select-only form writes
    assert _same_bytes(_ln_fwd(cuda, X, G, Bt, k0, SK, None, "gated")[0], SK)


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("gated_use", [False, True])
def test_layernorm_bwd_gate(cuda, deferred, gated_use):
    rows, cols = 9, 768
    torch.manual_seed(4)
    X = (torch.randn(rows, cols) * 2 + 0.5).to(BF).to(cuda)
    DY = torch.randn(rows, cols).to(BF).to(cuda)
    G, Bt = torch.randn(cols).to(cuda), torch.randn(cols).to(cuda)
    _, mean, rstd = _ln_fwd(cuda, X, G, Bt, None, None, None, "plain")
    dG0, dB0 = torch.randn(cols, device=cuda), torch.randn(cols, device=cuda)
    L, st = hip.lib(), hip.stream()

    def run(dy, x, mu, rs, keep, gate, entry="gate", drop=False):
        DX, DXD = _nan(rows, cols, device=cuda), _nan(rows, cols, device=cuda)
        dG, dB = dG0.clone(), dB0.clone()
        ws = hip.workspace(L.st5_layernorm_bwd_ws_bytes(rows, cols), cuda)
        hip.check(L.st5_layernorm_defer(1 if deferred else 0, st), "defer")
        try:
            a = (dy.data_ptr(), x.data_ptr(), G.data_ptr(), mu.data_ptr(), rs.data_ptr(), DX.data_ptr(), dG.data_ptr(), dB.data_ptr(), ws.data_ptr(),
                 rows, cols, DXD.data_ptr() if drop else None, 0.1 if drop else 0.0, 77 if drop else 0)
            if entry == "plain":
                hip.check(L.st5_layernorm_bwd(*a, hip.BF16, st), "bwd")
            else:
                hip.check(L.st5_layernorm_bwd_gate(*a, hip.ptr(keep), hip.ptr(gate), hip.BF16, st), "bwd gate")
            hip.check(L.st5_layernorm_flush(st), "flush")
        finally:
            hip.check(L.st5_layernorm_defer(0, st), "defer off")
        torch.cuda.synchronize()
        return DX, DXD, dG, dB

    k1, k0 = _keep(cuda, 1), _keep(cuda, 0)
    ref = run(DY, X, mean, rstd, None, None, "plain", drop=True)
    for got in (run(DY, X, mean, rstd, k1 if gated_use else None, None, drop=True), run(DY, X, mean, rstd, k1 if gated_use else None, k1, drop=True)):
        assert all(_same_bytes(a, b) for a, b in zip(ref, got))
    assert not _same_bytes(ref[2], dG0) and not _same_bytes(ref[3], dB0)
    N2, N1 = _nan(rows, cols, device=cuda), _nan(rows, dtype=torch.float32, device=cuda)
    dx, dxd, dG, dB = run(N2, N2, N1, N1, k0 if gated_use else None, k0, drop=True)
    assert _same_bytes(dG, dG0) and _same_bytes(dB, dB0), "a dropped LayerNorm changed dgamma / dbeta"
    assert torch.isnan(dx).all() and torch.isnan(dxd).all()


# ------------------------------------------------------------------------------------------------- 4. attention
_B, _H, _HD, _T, _S = 2, 2, 64, 70, 45
_D = _H * _HD


def _kpm(cuda, S):
    m = torch.zeros(_B, S, dtype=torch.uint8)
    m[1, S - 5:] = 1            # one padded row
    return m.to(cuda)


def test_self_attention_gate(cuda):
    torch.manual_seed(11)
    maxrel = 4                  # nb = 2 * maxrel = 8: the smallest table the entry accepts (nb % 8 == 0)
    qkv = (torch.randn(_B * _T, 3 * _D) * 0.5).to(BF).to(cuda)
    pe = (torch.randn(2 * maxrel, _HD) * 0.5).to(BF).to(cuda)
    dctx = torch.randn(_B * _T, _D).to(BF).to(cuda)
    kpm = _kpm(cuda, _T)
    seed = 4242
    tri = lambda t: ((t, 3 * _D, 0), (t, 3 * _D, _D), (t, 3 * _D, 2 * _D))

    def fwd(keep, x):
        with _gate(keep):
            return Fn._flash_fwd(*tri(x), _B, _H, _T, _T, _HD, pe, maxrel, kpm, False, 0.1, seed, save_qp=True)

    def bwd(keep, x, ctx, lse, qp, dc):
        dqkv = _nan(_B * _T, 3 * _D, device=cuda)
        with _gate(keep):
            dpe = Fn._flash_bwd(dc, ctx, lse, *tri(x), *tri(dqkv), _B, _H, _T, _T, _HD, pe, True, maxrel, kpm, False, 0.1, seed, qp=qp)
        torch.cuda.synchronize()
        return dqkv, dpe

    k1, k0 = _keep(cuda, 1), _keep(cuda, 0)
    ref, one = fwd(None, qkv), fwd(k1, qkv)
    torch.cuda.synchronize()
    assert all(_same_bytes(a, b) for a, b in zip(ref, one)) and not torch.isnan(ref[0]).any()
    rb, ob = bwd(None, qkv, *ref, dctx), bwd(k1, qkv, *ref, dctx)
    assert _same_bytes(rb[0], ob[0]) and _same_bytes(rb[1], ob[1]) and not torch.isnan(rb[0]).any() and float(rb[1].abs().max()) > 0
    Fn.set_layer_exit_nan_fill(True)        # the buffers _flash_fwd / _flash_bwd allocate start as NaN
    try:
        o, lse, qp = fwd(k0, qkv)
        torch.cuda.synchronize()
        assert torch.isnan(o).all() and torch.isnan(lse).all() and torch.isnan(qp).all(), "a dropped forward wrote o / lse / qp"
        xn = _nan(_B * _T, 3 * _D, device=cuda)
        dqkv, dpe = bwd(k0, xn, _nan(_B * _T, _D, device=cuda), _nan(_B * _H, _T, dtype=torch.float32, device=cuda), torch.full_like(ref[2], NAN),
                        _nan(_B * _T, _D, device=cuda))
    finally:
        Fn.set_layer_exit_nan_fill(False)
    assert torch.isnan(dqkv).all(), "a dropped self-attention backward wrote dq / dk / dv"
    assert dpe.shape == (2 * maxrel, _HD) and _same_bytes(dpe, torch.zeros_like(dpe)), "dPE of a dropped layer is not exact zeros"


def test_cross_attention_gate_shared_kv_slices(cuda):
    torch.manual_seed(12)
    ld = 3 * 2 * _D             # three layers' [K | V] side by side; this layer = slice 1
    koff = 2 * _D
    q = (torch.randn(_B * _T, _D) * 0.5).to(BF).to(cuda)
    kv = (torch.randn(_B * _S, ld) * 0.5).to(BF).to(cuda)
    dctx = torch.randn(_B * _T, _D).to(BF).to(cuda)
    kpm = _kpm(cuda, _S)
    seed = 777

    def fwd(keep, q_, kv_):
        with _gate(keep):
            return Fn._flash_fwd((q_, _D, 0), (kv_, ld, koff), (kv_, ld, koff + _D), _B, _H, _T, _S, _HD, None, 0, kpm, False, 0.1, seed)

    def bwd(keep, q_, kv_, ctx, lse, dc):
        dq, dkv = _nan(_B * _T, _D, device=cuda), _nan(_B * _S, ld, device=cuda)
        with _gate(keep):
            Fn._flash_bwd(dc, ctx, lse, (q_, _D, 0), (kv_, ld, koff), (kv_, ld, koff + _D), (dq, _D, 0), (dkv, ld, koff), (dkv, ld, koff + _D),
                          _B, _H, _T, _S, _HD, None, False, 0, kpm, False, 0.1, seed, dkv_live=keep is not None)
        torch.cuda.synchronize()
        return dq, dkv

    k1, k0 = _keep(cuda, 1), _keep(cuda, 0)
    ref, one = fwd(None, q, kv), fwd(k1, q, kv)
    torch.cuda.synchronize()
    assert _same_bytes(ref[0], one[0]) and _same_bytes(ref[1], one[1])
    rb, ob = bwd(None, q, kv, ref[0], ref[1], dctx), bwd(k1, q, kv, ref[0], ref[1], dctx)
    assert _same_bytes(rb[0], ob[0]) and _same_bytes(rb[1], ob[1])
    own = slice(koff, koff + 2 * _D)
    assert not torch.isnan(rb[1][:, own]).any() and torch.isnan(rb[1][:, :koff]).all() and torch.isnan(rb[1][:, koff + 2 * _D:]).all()
    Fn.set_layer_exit_nan_fill(True)
    try:
        o, lse, _ = fwd(k0, q, kv)
        torch.cuda.synchronize()
        assert torch.isnan(o).all() and torch.isnan(lse).all()
        dq, dkv = bwd(k0, _nan(_B * _T, _D, device=cuda), _nan(_B * _S, ld, device=cuda), _nan(_B * _T, _D, device=cuda),
                      _nan(_B * _H, _T, dtype=torch.float32, device=cuda), _nan(_B * _T, _D, device=cuda))
    finally:
        Fn.set_layer_exit_nan_fill(False)
    assert torch.isnan(dq).all(), "a dropped cross-attention backward wrote dq"
    assert _same_bytes(dkv[:, own], torch.zeros_like(dkv[:, own])), "the dropped layer's dK | dV slice is not exact zeros"
    assert torch.isnan(dkv[:, :koff]).all() and torch.isnan(dkv[:, koff + 2 * _D:]).all(), "a neighbour's slice was touched"


# ------------------------------------------------------------------------------------------------- 5. model level
_MODEL_SEED = 7      # (np / torch CPU seed; chosen so that the condition asserted in _loss_and_grads holds -- see the test's docstring)


def _loss_and_grads(cuda, exit_form, nan_fill, seed):
    from speecht5_amd.criterions import SpeechT5Criterion
    from speecht5_amd.speecht5 import T5TransformerModel
    from speecht5_amd.task import SpeechT5Task
    m, fx_s = load_golden("tiny_speech_pretrain.pt")
    _, fx_t = load_golden("tiny_text_pretrain.pt")
    args = Namespace(**m["args"])
    args.encoder_layerdrop = args.decoder_layerdrop = 0.4
    Fn.set_compute_dtype(BF)
    task = SpeechT5Task(args, Task().dicts)
    model = T5TransformerModel.build_model(args, task)
    torch.nn.Module.load_state_dict(model, m["state_dict"], strict=True)
    model = model.to(cuda).train()
    crit = SpeechT5Criterion(task, loss_weights=[10, 0.1], sync_logging=False)
    Fn.manual_seed(3)
    np.random.seed(seed)
    torch.manual_seed(seed)
    gates = []
    real = Fn.layerdrop_gate

    def spy(x, keep, exit=False):
        gates.append((keep, exit))
        return real(x, keep, exit)

    Fn._S.force_static = True
    Fn.set_layer_exit(exit_form)
    Fn.set_layer_exit_nan_fill(nan_fill)
    Fn.layerdrop_gate = spy
    try:
        out = []
        for fx in (fx_s, fx_t):
            del gates[:]
            model.zero_grad(set_to_none=True)
            loss, ss, _ = crit(model, to_dev(fx["sample"], cuda))
            (loss / ss).backward()
            torch.cuda.synchronize()
            flags = [(float(k), e) for k, e in gates]
            out.append((loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}, flags))
        return out
    finally:
        Fn.layerdrop_gate = real
        Fn._S.force_static = False
        Fn.set_layer_exit(True)
        Fn.set_layer_exit_nan_fill(False)
        Fn.weight_cache.clear()
        Fn.bf16_mirror.__init__()
        Fn.set_compute_dtype(torch.float32)


def test_exit_form_equals_select_only(cuda):
    """Tiny golden model, bf16, static form, LayerDrop 0.4, both micro-batches: loss and every parameter gradient of the exit form are
    byte-equal to the select-only form, also with every output of a gated launch NaN-filled.  The staged flags must show, in each
    micro-batch, a dropped and a kept encoder layer and a dropped and a kept decoder layer (2 + 2 layers: flags [enc0, enc1, dec0, dec1])."""
    sel = _loss_and_grads(cuda, False, False, _MODEL_SEED)
    ext = _loss_and_grads(cuda, True, False, _MODEL_SEED)
    nan = _loss_and_grads(cuda, True, True, _MODEL_SEED)
    for mb, (s, e, n) in enumerate(zip(sel, ext, nan)):
        print(f"micro-batch {mb}: staged keep flags {[f for f, _ in e[2]]}, gated {[x for _, x in e[2]]}, loss {float(e[0]):.6f}")
        flags = [f for f, _ in e[2]]
        assert len(flags) == 4 and all(x for _, x in e[2]), "every layer of the tiny model is expected to be gated in the exit form"
        assert not any(x for _, x in s[2]), "the switch did not turn the exit form off"
        assert sorted(flags[:2]) == [0.0, 1.0] and sorted(flags[2:]) == [0.0, 1.0], f"seed {_MODEL_SEED} does not drop one layer of each stack: {flags}"
        assert flags == [f for f, _ in s[2]] == [f for f, _ in n[2]]
        for other, what in ((e, "exit form"), (n, "exit form, NaN-filled outputs")):
            assert torch.isfinite(other[0]).all() and _same_bytes(s[0], other[0]), (what, "loss", float(s[0]), float(other[0]))
            assert set(s[1]) == set(other[1])
            for name, g in s[1].items():
                assert _same_bytes(g, other[1][name]), (what, name)


# ------------------------------------------------------------------------------------------------- 6. replay
def _tiny_update(cuda, graph, micro, n_updates):
    from speecht5_amd.criterions import SpeechT5Criterion
    from speecht5_amd.speecht5 import T5TransformerModel
    from speecht5_amd.task import SpeechT5Task
    from speecht5_amd.update import PretrainUpdate
    m, fx_s = load_golden("tiny_speech_pretrain.pt")
    _, fx_t = load_golden("tiny_text_pretrain.pt")
    args = Namespace(**m["args"])
    for k in ("dropout", "attention_dropout", "activation_dropout"):
        setattr(args, k, 0.1)
    args.encoder_layerdrop = args.decoder_layerdrop = 0.4
    Fn.set_compute_dtype(BF)
    task = SpeechT5Task(args, Task().dicts)
    model = T5TransformerModel.build_model(args, task)
    torch.nn.Module.load_state_dict(model, m["state_dict"], strict=True)
    model = model.to(cuda).train()
    crit = SpeechT5Criterion(task, loss_weights=[10, 0.1], sync_logging=False)
    Fn.manual_seed(21)
    np.random.seed(8)
    torch.manual_seed(8)
    upd = None
    try:
        upd = PretrainUpdate(task, model, crit, [to_dev(fx_s["sample"], cuda), to_dev(fx_t["sample"], cuda)], lr=1e-3, clip_norm=1.0,
                             graph=graph, micro=micro, device=cuda)
        if graph:
            upd.prepare_graph()
            for _ in range(n_updates - 2):
                upd.update()
            upd.finish()
        else:
            Fn._S.force_static = True
            for _ in range(n_updates):
                upd.eager_update()
        return upd.state()
    finally:
        Fn._S.force_static = False
        if upd is not None:
            upd.close()
        Fn.bf16_mirror.__init__()
        Fn.weight_cache.clear()
        Fn.set_layer_boundary_hook(None)
        Fn.set_compute_dtype(torch.float32)


def test_replayed_exit_form_equals_eager_in_turn(cuda):
    """PretrainUpdate on the tiny configuration, LayerDrop 0.4, exit form: 2 recorded + 4 replayed side-by-side updates == the same 6
    enqueued eagerly, in turn, in the static form: parameters and Adam moments byte for byte."""
    assert Fn.LAYER_EXIT
    ref = _tiny_update(cuda, False, "in_turn_2buf", 6)
    got = _tiny_update(cuda, True, "side_by_side", 6)
    assert ref[3] == got[3] == 6 and torch.isfinite(got[0]).all()
    for x, y, name in zip(ref[:3], got[:3], ("parameters", "first moment", "second moment")):
        assert _same_bytes(x, y), name
