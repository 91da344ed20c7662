"""Feature-specialised GEMM epilogues load their side operands (residual, pre-activation for GELU', old C) for the whole wave tile
ahead of the tile's first store.  The arithmetic is untouched, so the checks are bit for bit:

* NT kernels (128^2, half-height, phased 256^2) with F_RES, F_DROP|F_RES, F_DACT, F_BETA against the same call under
  st5_gemm_set_glds(0): the generic kernel and its run-time epilogue, which keeps the row-by-row order;
* grouped weight gradients (F_BETA, fp32 C) against exact arithmetic: the epilogue is one fp32 add, C == Z + X;
* the row-split layout (rpb != 0) through the convolution feature extractor's backward, whose GELU' data gradients are switched to
  the run-time form one launch at a time.

No call site of the library passes R or P aliasing C (DESIGN.md 4h lists them); F_BETA, which reads C itself, is covered here."""
import math

import pytest
import torch

from speecht5_amd import functional as Fn
from speecht5_amd import hip

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


class _switch:
    """One of the library's host-side A/B switches set inside the block, put back to `after` on the way out."""

    def __init__(self, name, value, after):
        self.fn, self.name, self.value, self.after = getattr(hip.lib(), name), name, value, after

    def __enter__(self):
        hip.check(self.fn(self.value), self.name)

    def __exit__(self, *exc):
        hip.check(self.fn(self.after), self.name)


# ------------------------------------------------------------------------------------------------- 1. NT kernels
_INPUTS = {}


def _nt_inputs(cuda, M, N, K):
    """Operands of one shape, made once and only read afterwards."""
    key = (M, N, K)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(7 * M + 3 * N + K)
        _INPUTS[key] = dict(A=(torch.randn(M, K, generator=g) * 0.5).to(BF).to(cuda), W=(torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF).to(cuda),
                            bias=torch.randn(N, generator=g).to(cuda), R=torch.randn(M, N, generator=g).to(BF).to(cuda),
                            P=torch.randn(M, N, generator=g).to(BF).to(cuda), C0=torch.randn(M, N, generator=g).to(BF).to(cuda))
    return _INPUTS[key]


def _run_nt(cuda, M, N, K, kind):
    t = _nt_inputs(cuda, M, N, K)
    C = torch.full((M, N), NAN, dtype=BF, device=cuda)
    if kind == "res":              # F_RES: data gradient plus the relayed residual gradient
        kw = dict(R=hip.operand(t["R"], N))
    elif kind == "drop_res":       # F_DROP | F_RES: bias, dropout, residual
        kw = dict(bias=t["bias"], dropout_p=0.1, seed=77, R=hip.operand(t["R"], N))
    elif kind == "dact":           # F_DACT: data gradient through the GELU
        kw = dict(P=hip.operand(t["P"], N), act=hip.ACT_GELU, flags=hip.DACT, alpha=0.5)
    elif kind == "beta":           # F_BETA: accumulate onto the old C
        C = t["C0"].clone()
        kw = dict(beta=1.0, bias=t["bias"])
    else:
        raise AssertionError(kind)
    hip.gemm(hip.operand(t["A"], K), hip.operand(t["W"], K), hip.operand(C, N), M, N, K, hip.BF16, **kw)
    torch.cuda.synchronize()
    return C


# (M, N, K, st5_gemm_set_nt_tile mode): 0 = the dispatcher's choice (128^2 here), 5 = the half-height kernel, 3 = the phased 256^2
# kernel, 2 = the first 256^2 kernel (run-time epilogue only)
_NT_CASES = [(200, 72, 128, 0),      # partial row and column tiles, shortest k-loop
             (264, 768, 768, 0),
             (64, 768, 768, 5),      # the half-height (m64) kernel
             (64, 768, 768, 0),
             (512, 512, 512, 2),
             (512, 512, 512, 3)]     # the phased kernel


@pytest.mark.parametrize("M,N,K,tile", _NT_CASES)
@pytest.mark.parametrize("kind", ["res", "drop_res", "dact", "beta"])
def test_nt_specialised_epilogue_equals_run_time_form(cuda, M, N, K, tile, kind):
    with _switch("st5_gemm_set_nt_tile", tile, 0):
        fast = _run_nt(cuda, M, N, K, kind)
    with _switch("st5_gemm_set_glds", 0, 1):
        ref = _run_nt(cuda, M, N, K, kind)
    assert not torch.isnan(ref).any() and not torch.isnan(fast).any()
    if kind != "beta":
        assert not _same_bytes(ref, _run_nt_plain(cuda, M, N, K)), "the side operand changed nothing: the case tests nothing"
    assert _same_bytes(fast, ref), f"{kind} {M}x{N}x{K} tile mode {tile}: {int((fast != ref).sum())} elements differ from the run-time form"


def _run_nt_plain(cuda, M, N, K):
    t = _nt_inputs(cuda, M, N, K)
    if "plain" not in t:
        C = torch.full((M, N), NAN, dtype=BF, device=cuda)
        hip.gemm(hip.operand(t["A"], K), hip.operand(t["W"], K), hip.operand(C, N), M, N, K, hip.BF16)
        torch.cuda.synchronize()
        t["plain"] = C
    return t["plain"]


# ------------------------------------------------------------------------------------------------- 2. grouped weight gradients
_TN = hip.A_KSTRIDED | hip.B_KSTRIDED | hip.OUT_F32


def _tn_problem(cuda, M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(K, M, generator=g) * 0.25).to(BF).to(cuda)      # dY [tokens, M], k-strided
    B = (torch.randn(K, N, generator=g) * 0.25).to(BF).to(cuda)      # X  [tokens, N], k-strided
    Z = torch.randn(M, N, generator=g).to(cuda)                      # the accumulator's old contents
    return A, B, Z


def _tn_group(cuda, probs, shapes, beta, start, gates=None):
    """One grouped launch; C starts as start[j] (cloned); returns the Cs."""
    out = [s.clone() for s in start]
    sums = [torch.zeros(M, device=cuda) for (M, _, _) in shapes]
    lst = []
    for j, ((A, B, _), C, (M, N, K)) in enumerate(zip(probs, out, shapes)):
        gt = gates[j] if gates else None
        lst.append((hip.operand(A, M), hip.operand(B, N), hip.operand(C, N), M, N, K, _TN, beta, sums[j], 0 if gt is None else gt.data_ptr()))
    hip.gemm_tn_group(lst, hip.BF16)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("M,N,K,tile,phased", [(256, 256, 512, 0, True), (136, 72, 256, 1, False)])
def test_grouped_weight_gradient_beta_is_one_exact_add(cuda, M, N, K, tile, phased):
    with _switch("st5_gemm_set_tn_group_tile", tile, 0):
        assert bool(hip.lib().st5_gemm_tn_group_is_phased(M, N, K)) == phased
        probs, shapes = [_tn_problem(cuda, M, N, K, seed=M + K)], [(M, N, K)]
        Z = probs[0][2]
        X = _tn_group(cuda, probs, shapes, 0.0, [torch.full_like(Z, NAN)])[0]
        C = _tn_group(cuda, probs, shapes, 1.0, [Z])[0]
    assert not torch.isnan(X).any() and X.abs().max().item() > 0
    assert _same_bytes(C, Z + X), f"{int((C != Z + X).sum())} elements of C differ from Z + X"


def test_grouped_weight_gradient_beta_group_of_three_with_a_dropped_layer(cuda):
    shapes = [(256, 256, 512), (256, 512, 576), (512, 256, 512)]     # K = 576: a ninth k-tile, no multiple of 128
    assert all(bool(hip.lib().st5_gemm_tn_group_is_phased(*s)) for s in shapes)
    probs = [_tn_problem(cuda, *s, seed=11 + i) for i, s in enumerate(shapes)]
    Zs = [p[2] for p in probs]
    keep1, keep0 = torch.tensor([1.0], device=cuda), torch.tensor([0.0], device=cuda)
    Xs = _tn_group(cuda, probs, shapes, 0.0, [torch.full_like(z, NAN) for z in Zs])
    Cs = _tn_group(cuda, probs, shapes, 1.0, Zs, gates=[keep1, keep0, None])
    assert _same_bytes(Cs[1], Zs[1]), "the dropped layer's accumulator changed"
    for j in (0, 2):
        assert _same_bytes(Cs[j], Zs[j] + Xs[j]), f"problem {j}: {int((Cs[j] != Zs[j] + Xs[j]).sum())} elements of C differ from Z + X"


# ------------------------------------------------------------------------------------------------- 3. row-split layout
def test_row_split_dact_through_the_conv_feature_extractor_backward(cuda, monkeypatch):
    """Layers 2 and 3 of a small feature extractor hand their data gradients through the GELU (F_DACT) into per-utterance blocks with
    halo rows: C and P are split every Lo (or Lo + 1) rows -- 49, 99 and 100 here, so blocks end inside 64-row wave tiles and the
    last tile is partial.  The same backward with exactly those launches on the run-time form must give the same gradients."""
    layers = [(128, 10, 5), (128, 3, 2), (128, 3, 2), (128, 2, 2)]
    g = torch.Generator().manual_seed(5)
    wav = torch.randn(2, 2000, generator=g).to(cuda)
    w0 = (torch.randn(128, 1, 10, generator=g) * 0.3).to(cuda).requires_grad_()
    gn_w = (1 + 0.1 * torch.randn(128, generator=g)).to(cuda).requires_grad_()
    gn_b = (0.1 * torch.randn(128, generator=g)).to(cuda).requires_grad_()
    ws = [(torch.randn(128, 128, k, generator=g) / math.sqrt(128 * k)).to(cuda).requires_grad_() for (_, k, _) in layers[1:]]
    params = [w0, gn_w, gn_b] + ws
    real_gemm, counted = hip.gemm, []

    def run(rt_for_dact):
        def gemm(*a, **kw):
            if kw.get("P") is not None and kw.get("flags", 0) & hip.DACT:
                counted.append(int(kw["P"].rpb))
                if rt_for_dact:
                    with _switch("st5_gemm_set_glds", 0, 1):
                        return real_gemm(*a, **kw)
            return real_gemm(*a, **kw)
        monkeypatch.setattr(hip, "gemm", gemm)
        for p in params:
            p.grad = None
        y = Fn.conv_feature_extractor(wav, layers, 1.0, w0, gn_w, gn_b, ws)
        dy = torch.sin(torch.arange(y.numel(), device=cuda, dtype=torch.float32)).reshape(y.shape).to(y.dtype)
        y.backward(dy)
        torch.cuda.synchronize()
        monkeypatch.setattr(hip, "gemm", real_gemm)
        return [p.grad.clone() for p in params]

    prev = Fn.compute_dtype()
    Fn.set_compute_dtype(BF)
    try:
        fast, ref = run(False), run(True)
    finally:
        Fn.set_compute_dtype(prev)
    assert sorted(counted) == sorted(2 * [49, 99, 100]), counted     # three row-split GELU' launches per backward
    for name, a, b in zip(["w0", "gn_w", "gn_b", "w1", "w2", "w3"], fast, ref):
        assert torch.isfinite(b).all() and b.abs().max().item() > 0, name
        assert _same_bytes(a, b), f"grad({name}): {int((a != b).sum())} elements differ from the run with run-time epilogues"
