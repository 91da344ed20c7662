"""csrc/conv0.hip (st5_conv0_gn_gelu_fwd / _bwd through the C ABI) against the fp64 truth of tests/conv0_reference.py, inside the
allowances that file derives -- on CORRELATED waveforms, where the layer's moment form cancels: AR(1), a 200 Hz tone, a DC offset,
a clip whose first moment chunk is all zeros, an all-zero and a constant clip, through difference, mean, quarter-rate cosine and all-zero
filters next to random ones.  White noise, the only input of the older tests, is the one input on which that cancellation is absent
(kappa ~ 1; here up to 1.5e5).

Geometry (conv0_reference.CASES): stride 5, k 10, L in {37, 256, 257, 1024, 1025, 1287} -- below one apply tile, at and one past the
256-frame apply / backward tile, at and one past the 1024-frame moment chunk, three ragged chunks -- with 3 trailing samples no frame
uses: at the odd L clip 1 starts 4-byte- but not 16-byte-aligned; k = 7 (padded taps of the KW = 10 instantiation); k = 12,
stride 4 (KW = 16, VALU only).  C = 32 (smallest matrix-core forward; VALU backward), 128 (smallest matrix-core backward), 8 (VALU
only).  Modes: fp32; bf16 under st5_conv0_set_mfma(0) and under (1) (restored to 1 afterwards).

Per case: the saved statistics inside the statistics allowance; every output element inside the forward bound, and finite; dW, dgamma,
dbeta -- accumulated onto non-zero seeds -- inside the backward bounds; a second call gives the same bits; NaN behind the last clip
never reaches a result and the guard row behind `out` is untouched.  Nothing in a bound comes from a kernel's output.  Each test prints
its worst error / bound per family (pytest -s); an MI355X run's figures are in profiles/conv0_fp64_ratios.txt."""
import functools

import pytest
import torch

from speecht5_amd import hip
from tests import conv0_reference as K

pytestmark = pytest.mark.gpu

SENT = -7.25          # exact in bf16
NAN_TAIL = 64


PARAMS = [pytest.param(c, m, id=f"{c.name}-{m}") for c in K.CASES for m in ("fp32", "bf16-mfma0", "bf16-mfma1")]


def _forward_form(case, mode):
    """The form the library runs: the matrix-core forward needs k <= 10 and C % 32 == 0; anything else is the VALU kernel under either
    setting of the switch (C = 8, k = 12: the dispatcher's fall-through is part of what mfma1 checks there)."""
    if mode == "fp32":
        return "fp32"
    return "bf16_mfma" if mode == "bf16-mfma1" and case.k <= 10 and case.C % 32 == 0 else "bf16_valu"


@functools.lru_cache(maxsize=None)
def _forward_reference(case):
    i = K.inputs(case)
    t = K.forward_truth(i.wav, i.w, i.gamma, i.beta, case.k, case.stride)
    return i, t, K.stats_allowance(t), K.apply_emulation(t, i.wav, i.w, i.gamma, i.beta)


@functools.lru_cache(maxsize=None)
def _backward_reference(case, dtype):
    i, t, _, _ = _forward_reference(case)
    return K.backward_truth(t, K.rnd(i.dY, dtype), K.GSCALE, i.dW0, i.dgamma0, i.dbeta0)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _run(case, mode, cuda):
    """One forward and one backward, twice; returns the first pass's results on the host."""
    i = K.inputs(case)
    dtype = torch.float32 if mode == "fp32" else torch.bfloat16
    B, S, L, C, k, stride = len(case.clips), K.samples(case), case.L, case.C, case.k, case.stride
    Ld = hip.lib()
    flat = torch.full((B * S + NAN_TAIL,), float("nan"), device=cuda)
    flat[:B * S] = i.wav.reshape(-1).to(cuda)
    assert flat.data_ptr() % 16 == 0          # (clip 1 starts S floats on: off a 16-byte boundary wherever S % 4 != 0)
    w, g, be = i.w.to(cuda).contiguous(), i.gamma.to(cuda), i.beta.to(cuda)
    dY = i.dY.to(dtype).to(cuda).contiguous()
    ws = hip.workspace(Ld.st5_conv0_ws_bytes(B, S, C, k, stride), cuda)
    passes = []
    try:
        if dtype == torch.bfloat16:
            hip.check(Ld.st5_conv0_set_mfma(1 if mode == "bf16-mfma1" else 0), "set_mfma")
        for _ in range(2):
            out = torch.full(((B * L + 1) * C,), SENT, dtype=dtype, device=cuda)
            stats = torch.full((B, C, 2), float("nan"), device=cuda)
            hip.check(Ld.st5_conv0_gn_gelu_fwd(flat.data_ptr(), w.data_ptr(), g.data_ptr(), be.data_ptr(), out.data_ptr(), stats.data_ptr(),
                                               ws.data_ptr(), B, S, C, k, stride, K.EPS, hip.dt(dtype), hip.stream()), "conv0 fwd")
            dW, dG, dB = i.dW0.to(cuda).contiguous(), i.dgamma0.to(cuda).contiguous(), i.dbeta0.to(cuda).contiguous()
            hip.check(Ld.st5_conv0_gn_gelu_bwd(flat.data_ptr(), w.data_ptr(), g.data_ptr(), be.data_ptr(), stats.data_ptr(), dY.data_ptr(),
                                               dW.data_ptr(), dG.data_ptr(), dB.data_ptr(), ws.data_ptr(), B, S, C, k, stride, K.GSCALE,
                                               hip.dt(dtype), hip.stream()), "conv0 bwd")
            torch.cuda.synchronize()
            passes.append((out.cpu(), stats.cpu(), dW.cpu(), dG.cpu(), dB.cpu()))
    finally:
        hip.check(Ld.st5_conv0_set_mfma(1), "set_mfma")
    tail = flat[B * S:].cpu()
    assert bool(torch.isnan(tail).all()), "NaN guard behind the waveform overwritten"
    for a, b, nm in zip(passes[0], passes[1], ("out", "stats", "dW", "dgamma", "dbeta")):
        assert torch.equal(_bits(a), _bits(b)), f"{nm}: two calls differ"
    out, stats, dW, dG, dB = passes[0]
    assert bool((out[B * L * C:].float() == SENT).all()), "guard row behind out overwritten"
    return out[:B * L * C].view(B, L, C), stats, dW, dG, dB


@pytest.mark.parametrize("case,mode", PARAMS)
def test_conv0_inside_the_derived_allowances(cuda, case, mode):
    out, stats, dW, dG, dB = _run(case, mode, cuda)
    form = _forward_form(case, mode)
    i, t, al, emu = _forward_reference(case)
    dtype = K.form_dtype(form)
    bwd_mfma = form == "bf16_mfma" and case.C % 128 == 0 and case.C <= 512
    bw = _backward_reference(case, dtype)
    fb = K.forward_bound(t, al, form, emu)
    bb = K.backward_bounds(t, bw, al, form if (form == "fp32" or bwd_mfma) else "bf16_valu", bwd_mfma)
    ex = K.eps_dominated(case)
    rm, rr = K.stats_ratio(t, al, stats[:, :, 0], stats[:, :, 1])
    pair = "+".join(case.clips)
    fig = []
    for b, fam in enumerate(case.clips):
        fig.append(("mean", fam, K.ratio(rm[b], torch.ones_like(rm[b]))))
        if (~ex[b]).any():
            fig.append(("rstd", fam, K.ratio(rr[b][~ex[b]], torch.ones_like(rr[b][~ex[b]]))))
        fig.append(("rstd eps-dominated", fam, K.ratio(rr[b][ex[b]], torch.ones_like(rr[b][ex[b]]))))
        fig.append(("out", fam, K.ratio(out[b].double() - t.out[b], fb[b])))
    fig.append(("dW", pair, K.ratio(dW.double() - (bw.dW0 + bw.dW), bb.dW)))
    fig.append(("dgamma", pair, K.ratio(dG.double() - (bw.dgamma0 + bw.dgamma), bb.dgamma)))
    fig.append(("dbeta", pair, K.ratio(dB.double() - (bw.dbeta0 + bw.dbeta), bb.dbeta)))
    bwd_form = "mfma" if bwd_mfma else "valu"
    for tensor, fam, r in fig:
        which = bwd_form if tensor in ("dW", "dgamma", "dbeta") else form
        print(f"\nconv0-ratio|{fam}|{form if which == form else form + '/bwd-' + which}|{tensor}|{r:.4f}|{case.name} {mode}", end="")
    if form == "bf16_mfma":          # how far the split-operand bound stands above one bf16 ulp of the output, and where
        for b, fam in enumerate(case.clips):
            live = ~ex[b]
            if live.any():
                wide = (fb[b] / (2.0 ** -8 * t.out[b].abs()).clamp_min(1e-30))[:, live]
                shift = (t.mean[b].abs() * t.rstd[b])[live].max().item()
                err_ulp = ((out[b].double() - t.out[b]).abs() / (2.0 ** -8 * t.out[b].abs()).clamp_min(1e-30))[:, live]
                print(f"\nconv0-split|{fam}|median bound / bf16 ulp {wide.median().item():.2f}|median error / bf16 ulp "
                      f"{err_ulp.median().item():.3f}|max abs(mean) rstd {shift:.1f}|{case.name}", end="")
    print()
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(stats).all())
    assert bool(torch.isfinite(dW).all()) and bool(torch.isfinite(dG).all()) and bool(torch.isfinite(dB).all())
    bad = [(tensor, fam, r) for tensor, fam, r in fig if not r <= 1.0]
    assert not bad, bad
