"""Pins tests/norm_reference.py (no GPU): the fp64 references against torch fp64 autograd, the counter / bucket restatements against
the tables of tests/attention_reference.py, every emulation's own error against a derived cap, and -- the evidence that the bars of
tests/test_norm_fp64_gpu.py can see a subtly wrong kernel -- every planted fault against those bars at one of the GPU case shapes.

Caps of the emulations: bf16 outputs 2^-6 (tests/test_attention_fp64_gpu.py); fp32 outputs 2^-24 x condition x 32, condition =
max |mean| / std over the rows for LayerNorm (a rounding of the mean moves the whole row by that much), 1 elsewhere, 32 covering the
handful of roundings per element and the 2^8 of the metric's floor on small rows; sums over rows: the any-order bound
gamma_rows * sum |t| (norm_reference.summation_floor with chain = rows)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_reference as A
from tests import norm_reference as R

BF, FP = torch.bfloat16, torch.float32
EPS = 1e-5


def _close64(a, b, tol=1e-10):
    a, b = a.double(), b.double()
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1e-30), (a - b).abs().max().item()


# ---- fp64 references == torch fp64 autograd ---------------------------------------------------------------------------------
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("rows,cols", [(5, 12), (33, 80), (7, 516)])
def test_layernorm_fp64_equals_autograd(rows, cols, gelu):
    x, gamma, beta, dy = R.ln_inputs(rows, cols, FP, "hard", seed=3)
    xa, ga, ba = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = F.layer_norm(xa, (cols,), ga, ba, float(np.float32(EPS)))
    y = F.gelu(y) if gelu else y
    y.backward(dy.double())
    yr, mean, rstd = R.layernorm_fwd(x, gamma, beta, EPS, gelu=gelu)
    _close64(yr, y.detach())
    _close64(mean, x.double().mean(1))
    _close64(rstd, 1 / torch.sqrt(x.double().var(1, unbiased=False) + float(np.float32(EPS))))
    g0, b0 = torch.randn(cols), torch.randn(cols)
    add = torch.randn(rows, cols)
    out = R.layernorm_bwd(dy, x, gamma, mean, rstd, beta=beta if gelu else None, addend=add, dgamma0=g0, dbeta0=b0, drop=(77, 0.5))
    _close64(out["dx"], xa.grad + add.double(), 1e-9)
    _close64(out["dgamma"], ga.grad + g0.double(), 1e-9)
    _close64(out["dbeta"], ba.grad + b0.double(), 1e-9)
    m = torch.from_numpy(R.keep_mask_rows(77, 0.5, rows, cols)).double() * A.inv_keep(0.5)
    _close64(out["dxd"], out["dx"] * m)
    gated = R.layernorm_bwd(dy, x, gamma, mean, rstd, keep=0.0, dgamma0=g0, dbeta0=b0)
    assert torch.all(gated["dx"] == 0) and torch.equal(gated["dgamma"], g0.double()) and torch.equal(gated["dbeta"], b0.double())
    assert torch.equal(R.layernorm_fwd(x, gamma, beta, EPS, keep=0.0, skip=add)[0], add.double())


@pytest.mark.parametrize("causal,T,S", [(False, 9, 21), (True, 12, 12), (True, 5, 19)])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_softmax_fp64_equals_autograd(causal, T, S, p):
    BH, H, maxrel, lds = 4, 2, 4, (S + 7) // 8 * 8
    scores, qp, kpm, dP, extra = R.softmax_inputs(BH, H, T, S, lds, maxrel, FP, lens=[S, S - 3], seed=5)
    sa, qa = scores[..., :S].double().requires_grad_(True), qp.double().requires_grad_(True)
    bk = A.buckets(T, S, maxrel)
    x = sa + torch.gather(qa, 2, bk[None].expand(BH, T, S))
    vis = torch.stack([A.visible(T, S, kpm[b // H], causal) for b in range(BH)])
    Pt = torch.softmax(x.masked_fill(~vis, float("-inf")), -1)
    M = torch.ones(BH, T, S, dtype=torch.float64)
    if p > 0:
        M = torch.from_numpy(R.keep_mask_softmax(99, p, BH * T, S, lds)).view(BH, T, S).double() * A.inv_keep(p)
    ((Pt * M * dP[..., :S].double()).sum() + (Pt * extra.double()).sum()).backward()
    r = R.softmax_fwd_bwd(scores, qp, kpm, dP, extra, BH, H, T, S, lds, maxrel, causal, p, 99)
    _close64(r["P"][..., :S], Pt.detach())
    _close64(r["PD"][..., :S], (Pt * M).detach())
    _close64(r["dS"][..., :S], sa.grad, 1e-9)
    _close64(r["dQP"], qa.grad, 1e-9)
    assert torch.all(r["P"][..., S:] == 0) and torch.all(r["dS"][..., S:] == 0) and r["live"].all()


def test_softmax_fully_padded_item_is_zero():
    BH, H, T, S, lds, maxrel = 4, 2, 3, 8, 8, 4
    scores, qp, kpm, dP, extra = R.softmax_inputs(BH, H, T, S, lds, maxrel, FP, lens=[8, 0])
    for emulate in (False, True):
        r = R.softmax_fwd_bwd(scores, qp, kpm, dP, extra, BH, H, T, S, lds, maxrel, False, 0.1, 5, dtype=FP, emulate=emulate)
        for nm in ("P", "PD", "dS", "dQP"):
            assert torch.all(r[nm][2:] == 0), nm
        assert r["live"][:2].all() and not r["live"][2:].any()


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("tanh", [True, False])
def test_batchnorm_fp64_equals_autograd(training, tanh):
    rows, C = 37, 12
    x, dy, gamma, beta, res, rmean, rvar = R.bn_inputs(rows, C)
    xa, ga, ba = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    rm, rv = rmean.double().clone(), rvar.double().clone()
    y = F.batch_norm(xa, rm, rv, ga, ba, training, 0.1, float(np.float32(EPS)))
    y = torch.tanh(y) if tanh else y
    y.backward(dy.double())
    f = R.batchnorm_fwd(x, gamma, beta, rmean, rvar, 3, 0.1, EPS, training, tanh, 0.0, 0, residual=res)
    _close64(f["y"], y.detach() + res.double())
    _close64(f["running_mean"], rm, 1e-7)       # (momentum is the fp32 0.1 in the reference, as the kernel receives it)
    _close64(f["running_var"], rv, 1e-7)
    assert f["nbt"] == (4 if training else 3)
    g0, b0 = torch.randn(C), torch.randn(C)
    b = R.batchnorm_bwd(x, dy, f["mean"], f["rstd"], gamma, beta, training, tanh, 0.0, 0, dgamma0=g0, dbeta0=b0)
    _close64(b["dx"], xa.grad, 1e-9)
    _close64(b["dgamma"], ga.grad + g0.double(), 1e-9)
    _close64(b["dbeta"], ba.grad + b0.double(), 1e-9)
    # dropout: the mask multiplies the activated value, the same mask the gradient
    fd = R.batchnorm_fwd(x, gamma, beta, rmean, rvar, 0, 0.1, EPS, training, tanh, 0.5, 11)
    m = torch.from_numpy(R.keep_mask_rows(11, 0.5, rows, C)).double() * A.inv_keep(0.5)
    _close64(fd["y"], (f["y"] - res.double()) * m)


# ---- restatements ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 100, 499, 513, 999, 4093])
def test_counter_and_bucket_restatements_equal_attention_reference(S):
    lds = (S + 7) // 8 * 8
    assert R.drop_row_stride(lds) == A.attention_row_stride(S)
    BH, T = 3, 5
    assert np.array_equal(R.keep_mask_softmax(4242, 0.1, BH * T, S, lds).reshape(BH, T, S), A.keep_mask_attention(4242, 0.1, BH, T, S))
    assert torch.equal(R.bucket_table(T + 170, S, 160), A.buckets(T + 170, S, 160))
    assert np.array_equal(R.keep_mask_rows(7, 0.5, 3, S), A.keep_mask_flat(7, 0.5, np.arange(3 * S, dtype=np.uint64)).reshape(3, S))


def test_lane_order_sum_and_block_geometry():
    v = np.arange(1, 3 * 516 + 1, dtype=np.float32).reshape(3, 516)          # integers: every order is exact
    for group in (4, 8):
        assert np.array_equal(R.lane_order_sum(v, group), v.sum(1, dtype=np.float64).astype(np.float32))
    w = np.random.default_rng(0).standard_normal((4, 2052)).astype(np.float32)
    assert np.abs(R.lane_order_sum(w, 8) - w.sum(1, dtype=np.float64)).max() <= 24 * R.U32 * np.abs(w).sum(1).max()
    assert R.ln_blocks(3992) == 250 and R.ln_trips(3992) == (1, 1)
    assert R.ln_blocks(8192) == 256 and R.ln_trips(8192) == (2, 2)
    assert R.ln_blocks(8200) == 171 and R.ln_trips(8200) == (2, 3)
    assert R.ln_trips(16408)[0] >= 3 and R.ln_trips(300, 2)[1] >= 5
    assert R.bn_geometry(111, 64)[1] == 1 and R.bn_geometry(19200, 256) == (4, 64) and R.bn_geometry(2, 4) == (256, 1)


# ---- the emulations' own error ----------------------------------------------------------------------------------------------
def _cap(dtype, cond=1.0):
    return R.EMU_CAP_BF16 if dtype == BF else R.U32 * cond * 32


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("family", ["randn", "hard"])
@pytest.mark.parametrize("rows,cols", [(17, 768), (300, 516), (64, 2052)])
def test_layernorm_emulation_error_is_nonzero_and_capped(rows, cols, family, dtype):
    x, gamma, beta, dy = R.ln_inputs(rows, cols, dtype, family)
    cond = R.ln_condition(x)
    y, mean, rstd = R.layernorm_fwd(x, gamma, beta, EPS)
    ye, me, re = R.layernorm_fwd(x, gamma, beta, EPS, dtype=dtype, emulate=True)
    ref = R.layernorm_bwd(dy, x, gamma, mean, rstd)
    emu = R.layernorm_bwd(dy, x, gamma, me, re, dtype=dtype, emulate=True)
    for nm, e, r, cap in (("y", ye, y, _cap(dtype, cond)), ("mean", me, mean, R.U32 * 32), ("rstd", re, rstd, R.U32 * 32),
                          ("dx", emu["dx"], ref["dx"], _cap(dtype, cond))):
        err = R.row_metric(e, r)
        assert 0 < err <= cap, f"{nm}: {err:.3e} cap {cap:.3e} (condition {cond:.1f})"
    for nm in ("dgamma", "dbeta"):
        err = (emu[nm].double() - ref[nm]).abs()
        # (dbeta of a few bf16 rows is an exact fp32 sum: only dgamma, whose terms are rounded products, must differ from fp64)
        assert (err.max() > 0 or nm == "dbeta") and torch.all(err <= R.summation_floor(ref["abs_" + nm] * max(cond, 1.0), rows)), nm


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("scale", [1.0, 80.0])
def test_softmax_emulation_error_is_nonzero_and_capped(dtype, scale):
    BH, H, T, S, lds, maxrel = 6, 3, 5, 999, 1000, 160
    scores, qp, kpm, dP, extra = R.softmax_inputs(BH, H, T, S, lds, maxrel, dtype, scale=scale, lens=[S, 700])
    args = (scores, qp, kpm, dP, extra, BH, H, T, S, lds, maxrel, False, 0.1, 31)
    ref, emu = R.softmax_fwd_bwd(*args), R.softmax_fwd_bwd(*args, dtype=dtype, emulate=True)
    # the exponent's argument is rounded once at magnitude <= 2 * 1.5 * 80 * log2 e: condition of exp
    cond = 1.0 if dtype == BF else max(1.0, 4 * scale * 1.4427)
    for nm in ("P", "PD", "dS", "dQP"):
        err = R.row_metric(emu[nm], ref[nm])
        assert err > 0, nm
        assert torch.all(emu[nm][..., S:] == 0) if nm != "dQP" else True
        if scale == 1 or nm in ("P", "PD"):
            assert err <= _cap(dtype, cond), f"{nm}: {err:.3e}"
    if scale > 1:
        # Rows are nearly one-hot: dS = P (g - P . g) cancels to (1 - max P) of its terms, so the cap is the first-order bound itself.
        # With dP = relative error of a probability (u of the type + the exponent's 2^-24 * cond): |d dS_j| <= dP (2 |dS_j| + P_j sum |g P|)
        # per element, the row norm and the bucket sums (1-norm) follow; x 4 for the final roundings.
        dPr = R.unit(dtype) + R.U32 * cond
        M = torch.from_numpy(R.keep_mask_softmax(31, 0.1, BH * T, S, lds)).view(BH, T, S).double() * A.inv_keep(0.1)
        g = dP[..., :S].double() * M + extra.double()
        Pf, dSf = ref["P"][..., :S], ref["dS"][..., :S]
        gp = (g * Pf).abs().sum(2)
        b_dS = 4 * dPr * (2 * dSf.norm(dim=2) + Pf.norm(dim=2) * gp)
        b_dQP = 4 * dPr * (2 * dSf.abs().sum(2) + gp)
        assert torch.all((emu["dS"].double() - ref["dS"]).norm(dim=2) <= b_dS)
        assert torch.all((emu["dQP"].double() - ref["dQP"]).norm(dim=2) <= b_dQP)


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("training", [True, False])
def test_batchnorm_emulation_error_is_nonzero_and_capped(dtype, training):
    rows, C = 4097, 80
    x, dy, gamma, beta, res, rmean, rvar = R.bn_inputs(rows, C)
    a = (x, gamma, beta, rmean, rvar, 0, 0.1, EPS, training, True, 0.5, 3)
    ref, emu = R.batchnorm_fwd(*a, residual=res.to(dtype)), R.batchnorm_fwd(*a, residual=res.to(dtype), y_f32=False, dtype=dtype, emulate=True)
    # channel with mean 50, spread 0.1: the fp32 mean and x - mean carry 2^-24 * 50 / 0.1
    cond = 500.0
    for nm in ("y", "mean", "rstd", "running_mean", "running_var"):
        err = R.row_metric(emu[nm], ref[nm])
        assert (0 < err or not training) and err <= (_cap(dtype, cond) if nm == "y" else R.U32 * 32), f"{nm}: {err:.3e}"
    rb = R.batchnorm_bwd(x, dy, ref["mean"], ref["rstd"], gamma, beta, training, True, 0.5, 3)
    eb = R.batchnorm_bwd(x, dy, emu["mean"], emu["rstd"], gamma, beta, training, True, 0.5, 3, dtype=dtype, emulate=True)
    assert 0 < R.row_metric(eb["dx"], rb["dx"]) <= _cap(dtype, cond)
    for nm in ("dgamma", "dbeta"):
        assert 0 < R.row_metric(eb[nm], rb[nm]) <= R.U32 * cond * 32, nm


# ---- planted faults: each must fail the bars of tests/test_norm_fp64_gpu.py at one of its case shapes -----------------------------
def _ln_case(rows, cols, dtype, family, fwd_fault=None, bwd_fault=None, max_blocks=256):
    x, gamma, beta, dy = R.ln_inputs(rows, cols, dtype, family)
    y, mean, rstd = R.layernorm_fwd(x, gamma, beta, EPS)
    ref = dict(R.layernorm_bwd(dy, x, gamma, mean, rstd), y=y, mean=mean, rstd=rstd)
    out = []
    for ff, bf in ((None, None), (fwd_fault, bwd_fault)):
        ye, me, re = R.layernorm_fwd(x, gamma, beta, EPS, dtype=dtype, emulate=True, fault=ff)
        out.append(dict(R.layernorm_bwd(dy, x, gamma, me, re, dtype=dtype, emulate=True, fault=bf, max_blocks=max_blocks), y=ye, mean=me, rstd=re))
    return ref, out[0], out[1]


def _floor(ref, nm, rows, max_blocks=256):
    return R.summation_floor(ref["abs_" + nm], R.ln_sum_chain(rows, max_blocks))


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("rows,max_blocks", [(8192, 256), (8200, 256), (300, 2)])
def test_fault_trip_tail_rows_missing_from_dgamma_dbeta(rows, max_blocks, dtype):
    ref, emu, bad = _ln_case(rows, 768, dtype, "randn", bwd_fault="trip_tail", max_blocks=max_blocks)
    for nm in ("dgamma", "dbeta"):
        assert R.passes(emu[nm], ref[nm], emu[nm], floor=_floor(ref, nm, rows, max_blocks))[0]
        assert not R.passes(bad[nm], ref[nm], emu[nm], floor=_floor(ref, nm, rows, max_blocks))[0], nm
    assert torch.equal(bad["dx"], emu["dx"])      # nothing else sees it: dgamma / dbeta are the only witnesses


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cols", [80, 516, 1028])      # (1280 = 5 full chunks of the NV = 6 kernel: nothing partial to skip)
def test_fault_last_vector_chunk_skipped(cols, dtype):
    ref, emu, bad = _ln_case(17, cols, dtype, "hard", fwd_fault="skip_last_chunk")
    assert not R.passes(bad["mean"], ref["mean"], emu["mean"])[0]
    assert not R.passes(bad["y"], ref["y"], emu["y"])[0]


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp32"])
def test_fault_previous_rows_mean(dtype):
    ref, emu, bad = _ln_case(17, 768, dtype, "randn", fwd_fault="prev_row_mean")
    assert not R.passes(bad["mean"], ref["mean"], emu["mean"])[0]
    assert not R.passes(bad["y"], ref["y"], emu["y"])[0] and not R.passes(bad["dx"], ref["dx"], emu["dx"])[0]


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cols", [80, 768, 2048, 4096])
def test_fault_unbiased_variance(cols, dtype):
    ref, emu, bad = _ln_case(16, cols, dtype, "randn", fwd_fault="unbiased_var")
    assert not R.passes(bad["rstd"], ref["rstd"], emu["rstd"])[0]          # rstd is fp32 in both modes: 1 / (2 cols) >> 2^-24
    if dtype == FP:                                                          # (bf16 y: 1 / (2 cols) is below the type's own rounding)
        assert not R.passes(bad["y"], ref["y"], emu["y"])[0]


def _sm_case(T, S, lds, dtype, causal, p, fault):
    BH, H, maxrel = 6, 3, 160
    scores, qp, kpm, dP, extra = R.softmax_inputs(BH, H, T, S, lds, maxrel, dtype, lens=[S, S - S // 5])
    args = (scores, qp, kpm, dP, extra, BH, H, T, S, lds, maxrel, causal, p, 4321)
    return (R.softmax_fwd_bwd(*args), R.softmax_fwd_bwd(*args, dtype=dtype, emulate=True),
            R.softmax_fwd_bwd(*args, dtype=dtype, emulate=True, fault=fault))


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("fault,T", [("clip_low", 70), ("clip_high", 331)])
def test_fault_bucket_clip_off_by_one(fault, T, dtype):
    ref, emu, bad = _sm_case(T, 499, 504, dtype, False, 0.0, fault)
    assert R.passes(emu["P"], ref["P"], emu["P"])[0]
    fullest = int(torch.bincount(R.bucket_table(T, 499, 160).reshape(-1)).max())
    floor = R.summation_floor(ref["abs_dQP"], fullest).norm(dim=-1)                    # the floor the GPU test gives dQP
    assert R.passes(emu["dQP"], ref["dQP"], emu["dQP"], floor=floor)[0]
    assert not R.passes(bad["P"], ref["P"], emu["P"])[0] and not R.passes(bad["dQP"], ref["dQP"], emu["dQP"], floor=floor)[0]


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp32"])
def test_fault_causal_limit_without_offset(dtype):
    ref, emu, bad = _sm_case(70, 499, 504, dtype, True, 0.0, "causal_no_offset")
    assert not R.passes(bad["P"], ref["P"], emu["P"])[0] and not R.passes(bad["dS"], ref["dS"], emu["dS"])[0]


@pytest.mark.parametrize("S,lds", [(499, 504), (999, 1000), (4093, 4096)])
def test_fault_dropout_counter_stride(S, lds):
    ref, emu, bad = _sm_case(5, S, lds, FP, False, 0.1, "stride_S")
    keep = R.keep_mask_softmax(4321, 0.1, 6 * 5, S, lds).reshape(6, 5, S)
    assert R.dropout_pattern_ok(emu["PD"], emu["P"], keep, 0.1, S)
    assert not R.dropout_pattern_ok(bad["PD"], bad["P"], keep, 0.1, S)


@pytest.mark.parametrize("rows,C", [(4097, 80), (19200, 256), (19200, 1024)])
def test_fault_batchnorm_partial_block_left_out(rows, C):
    x, dy, gamma, beta, res, rmean, rvar = R.bn_inputs(rows, C)
    a = (x, gamma, beta, rmean, rvar, 0, 0.1, EPS, True, True, 0.0, 0)
    ref, emu, bad = R.batchnorm_fwd(*a), R.batchnorm_fwd(*a, emulate=True), R.batchnorm_fwd(*a, emulate=True, fault="skip_block")
    for nm in ("mean", "rstd", "running_mean", "running_var", "y"):
        assert R.passes(emu[nm], ref[nm], emu[nm])[0]
        assert not R.passes(bad[nm], ref[nm], emu[nm])[0], nm


def test_fault_halo_one_row_short():
    L, pad, C, nbatch = 600, 2, 80, 3
    y = torch.randn(nbatch * L, C)
    bstride = (L + 2 * pad) * C + 24
    good, bad = R.place_rows(y, L, pad, bstride, -7.25, BF), R.place_rows(y, L, pad, bstride, -7.25, BF, fault="halo_short")
    assert torch.equal(R.extract_rows(good, nbatch, C, L, pad, bstride), y.to(BF))
    assert R.mapped_layout_ok(good, nbatch, C, L, pad, bstride, -7.25)
    assert not R.mapped_layout_ok(bad, nbatch, C, L, pad, bstride, -7.25)
