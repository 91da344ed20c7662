"""tests/gemm_reference.py checked without a GPU: the fp64 form against torch's own double arithmetic, the addressing gather against
plain slicing, the emulation against its own bar and a per-dtype cap derived from the formats, every named fault shown to FAIL the bar
(so a kernel that is wrong in that way cannot pass tests/test_gemm_fp64_gpu.py), and the condition under which the dropout cases decide
every mask bit by value."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_reference as A
from tests import gemm_reference as G

BF, FP = torch.bfloat16, torch.float32
DTYPES, IDS = [BF, FP], ["bf16", "fp32"]


def _judge(got, ref, emu, what="C"):
    if what == "asum":
        return G.judge(got.asum, ref.asum, emu.asum, ref.S_asum, ref.K_asum, FP)
    if what == "Cpre":
        return G.judge(got.Cpre, ref.Cpre, emu.Cpre, ref.S_pre, ref.chain, ref.pre_dtype)
    return G.judge(got.C, ref.C, emu.C, ref.S, ref.chain, ref.c_dtype, ref.extra)


def _both(p, dtype):
    ref, emu = G.gemm(p, dtype), G.gemm(p, dtype, emulate=True)
    ref.K_asum, ref.pre_dtype = p.K + 1, dtype
    return ref, emu


# ---- the fp64 form is the formula ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fp64_form_against_torch(dtype):
    """C = GELU(0.5 A B^T + bias) + R + C_old and Cpre, and the DACT form, against F.linear / F.gelu / autograd in double."""
    M, N, K = 63, 72, 24
    p = G.case(M, N, K, dtype, "all", p_drop=0.1)
    p.alpha = 0.5
    v = G.inputs(M, N, K, bias_offset=3.0)
    a, b, r, c0 = (v[k][0].to(dtype).double() for k in ("A", "B", "R", "C0"))
    pre = 0.5 * F.linear(a, b) + v["bias"].double()
    keep = torch.from_numpy(A.keep_mask_flat(77, 0.1, np.arange(M * N, dtype=np.uint64).reshape(M, N)))
    want = F.gelu(pre) * keep * A.inv_keep(0.1) + r + c0
    ref = G.gemm(p, dtype)
    assert torch.allclose(ref.C[0], want, rtol=1e-13, atol=1e-13) and torch.allclose(ref.Cpre[0], pre, rtol=1e-13, atol=1e-13)
    for kind, fn in (("dact", F.gelu), ("d_tanh", torch.tanh), ("d_relu", F.relu), ("d_lrelu01", lambda x: F.leaky_relu(x, float(np.float32(0.1))))):
        p = G.case(M, N, K, dtype, kind)
        v = G.inputs(M, N, K)
        x = v["P"][0].to(dtype).double().requires_grad_(True)
        fn(x).sum().backward()
        want = p.alpha * F.linear(v["A"][0].to(dtype).double(), v["B"][0].to(dtype).double()) * x.grad
        assert torch.allclose(G.gemm(p, dtype).C[0], want, rtol=1e-12, atol=1e-13), kind
    p = G.wgrad_case(136, 72, 256, dtype, beta=1.0, asum=True)
    v = G.inputs(136, 72, 256)
    a, b = v["A"][0].to(dtype).double(), v["B"][0].to(dtype).double()
    ref = G.gemm(p, dtype)
    assert torch.allclose(ref.C[0], a @ b.t() + v["C0"][0].double(), rtol=1e-13, atol=1e-13)
    assert torch.allclose(ref.asum, v["asum0"].double() + a.sum(1), rtol=1e-13, atol=1e-13)


# ---- the addressing gather is the header's formula ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride", [(3, 2), (2, 2)])
def test_gather_agrees_with_slicing_on_the_conv_layout(k, stride):
    """Strided Conv1d as implicit GEMM on channels-last rows (test_ops_gpu.py::test_gemm_conv1d_channels_last): row (b, t) of A is the
    k * Cin elements from x[b, t * stride]; rows overlap."""
    B, L, Cin = 3, 101, 64
    Lo = (L - k) // stride + 1
    x = torch.randn(B, L, Cin, generator=torch.Generator().manual_seed(11))
    op = G.Op(x.reshape(-1), stride * Cin, rpb=Lo, bstride=L * Cin)
    got = G.gather_ab(op, B * Lo, k * Cin, False)
    want = x.unfold(1, k, stride).permute(0, 1, 3, 2).reshape(B * Lo, k * Cin)       # [B, Lo, Cin, k] -> [B, Lo, k, Cin]
    assert torch.equal(got, want)
    conv = F.conv1d(x.transpose(1, 2).double(), torch.ones(1, Cin, k, dtype=torch.float64), stride=stride)[:, 0].reshape(-1)
    assert torch.allclose(got.double().sum(1), conv, rtol=1e-12, atol=1e-12)


def test_gather_agrees_with_slicing_on_heads_segments_and_k_strided():
    g = torch.Generator().manual_seed(5)
    Bn, H, T, hd = 2, 3, 70, 64
    d = H * hd
    qkv = torch.randn(Bn * T, 3 * d, generator=g)
    x = qkv.view(Bn, T, 3, H, hd)
    for which in range(3):      # q, k, v of (batch, head) z out of the fused projection buffer: zs0 = one batch, zs1 = one head, off = q / k / v
        op = G.Op(qkv.reshape(-1), 3 * d, off=which * d, zs0=T * 3 * d, zs1=hd)
        for z in range(Bn * H):
            assert torch.equal(G.gather_ab(op, T, hd, False, z, H), x[z // H, :, which, z % H])
    # v as the k-strided B operand of P.V: outer = key, inner = head channel
    op = G.Op(qkv.reshape(-1), 3 * d, off=2 * d, zs0=T * 3 * d, zs1=hd)
    assert torch.equal(G.gather_ab(op, hd, T, True, 4, H), x[1, :, 2, 1].t())
    # grouped pos-conv (test_gemm_grouped_posconv): k taps of cg channels out of rows C wide, group z at zs0 = cg
    Tp, C, Gr, k = 66, 64, 4, 16
    cg = C // Gr
    xp = torch.randn(2, Tp, C, generator=g)
    op = G.Op(xp.reshape(-1), C, rpb=50, bstride=Tp * C, seg=cg, seg_stride=C, zs0=cg)
    for z in range(Gr):
        want = xp[:, :, z * cg:(z + 1) * cg].unfold(1, k, 1)[:, :50].permute(0, 1, 3, 2).reshape(100, k * cg)
        assert torch.equal(G.gather_ab(op, 100, k * cg, False, z, 1), want)
    # row-split C with halo rows
    buf = torch.arange(4 * 52 * 144, dtype=torch.float32)
    p = G.problem(None, None, None, 200, 136, 8)
    got = G.gather_c(G.Op(buf, 144, rpb=50, bstride=52 * 144), p)[0]
    assert torch.equal(got, buf.view(4, 52, 144)[:, :50, :136].reshape(200, 136))


# ---- emulation: inside its own bar, capped from the formats --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", G.KINDS + G.RT_KINDS)
def test_emulation_passes_its_own_bar_and_is_capped(dtype, kind):
    """|emulation - fp64| <= 1 ulp of the output type (one rounding is ulp / 2; the rest is what the fp32 chain in front of it moved the
    value across a rounding boundary) + the summation bound (+ the documented polynomial error): nothing measured."""
    for M, N, K, layout in ((63, 72, 24, "plain"), (63, 83, 24, "plain"), (63, 72, 24, "unaligned"), (200, 136, 300, "plain")):
        p = G.case(M, N, K, dtype, kind, layout=layout)
        ref, emu = _both(p, dtype)
        assert emu.fast == (layout == "plain" and N % 8 == 0)
        for what in ("C",) + (("Cpre",) if p.Cpre is not None else ()):
            ok, ek, ee, ratio = _judge(emu, ref, emu, what)
            assert ok and ratio <= 1.0, (what, ratio)
        cap = G.ulp_out(ref.C, ref.c_dtype) + G.NR.summation_floor(ref.S, ref.chain, ref.extra)
        assert bool(((emu.C - ref.C).abs() <= cap).all()), (M, N, K, layout, ((emu.C - ref.C).abs() / cap).max().item())
        if p.Cpre is not None:
            cap = G.ulp_out(ref.Cpre, dtype) + G.NR.summation_floor(ref.S_pre, ref.chain)
            assert bool(((emu.Cpre - ref.Cpre).abs() <= cap).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_emulated_asum_is_capped(dtype):
    p = G.wgrad_case(136, 72, 256, dtype, asum=True)
    ref, emu = _both(p, dtype)
    assert _judge(emu, ref, emu, "asum")[0]
    assert bool(((emu.asum - ref.asum).abs() <= G.ulp_out(ref.asum, FP) + G.NR.summation_floor(ref.S_asum, ref.K_asum)).all())


# ---- every named fault fails the bar ---------------------------------------------------------------------------------------------
def _fault_case(fault, dtype):
    """(problem, judged tensor): the smallest shape of the family the fault belongs to."""
    if fault == "a_last_k":
        return G.case(63, 72, 8, dtype, "plain"), "C"
    if fault == "k_tail_poison":
        return G.case(63, 72, 24, dtype, "plain"), "C"
    if fault == "bias_shift":
        return G.case(63, 83, 24, dtype, "bias"), "C"
    if fault == "alpha_after_bias":
        return G.case(63, 72, 24, dtype, "alpha_bias"), "C"
    if fault == "r_row":
        return G.case(200, 136, 128, dtype, "res", layout="rowsplit", rpb=50), "C"
    if fault == "mask_shift":
        return G.case(63, 136, 128, dtype, "drop_res"), "C"
    if fault == "mask_no_base":
        return G.case(63, 136, 128, dtype, "drop_res", batch=3, zdiv=3), "C"
    if fault == "beta_before_drop":
        return G.case(63, 72, 24, dtype, "all"), "C"
    if fault == "cpre_post":
        return G.case(63, 72, 24, dtype, "gelu_pre"), "Cpre"
    return G.wgrad_case(136, 72, 256, dtype, asum=True), "asum"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", G.FAULTS)
def test_every_named_fault_fails_the_bar(dtype, fault):
    p, what = _fault_case(fault, dtype)
    ref, emu = _both(p, dtype)
    bad = G.gemm(p, dtype, emulate=True, fault=fault)
    assert _judge(emu, ref, emu, what)[0]
    ok, ek, ee, ratio = _judge(bad, ref, emu, what)
    assert not ok and ratio > 2 * G.BAR, (fault, ratio)


def test_bias_shift_fails_on_the_fast_layout_too():
    p = G.case(63, 72, 24, BF, "bias")
    ref, emu = _both(p, BF)
    assert not _judge(G.gemm(p, BF, emulate=True, fault="bias_shift"), ref, emu)[0]


# ---- dropout: the comparison by value decides every mask bit ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_wrong_mask_bit_is_far_outside_the_tolerance(dtype):
    """In the reference alone, for EVERY problem with dropout that tests/test_gemm_fp64_gpu.py runs (gemm_reference.all_dropout_problems:
    the same shape lists): the share of elements whose |x| / (1 - p) is below 8 x their tolerance stays <= 1 % (the bias of these cases is
    3 + 0.5 N(0, 1) against products of spread 0.25), and the mask itself keeps about 1 - p."""
    n = 0
    for name, p in G.all_dropout_problems(dtype):
        ref, emu = _both(p, dtype)
        tol = G.tolerance(ref.C, emu.C, ref.S, ref.chain, ref.c_dtype, ref.extra)
        assert G.mask_decides(ref, tol, p.dropout_p) <= 0.01, name
        if ref.keep.numel() > 4096:
            assert abs(ref.keep.double().mean().item() - (1 - p.dropout_p)) < 0.02, name
        n += 1
    assert n == 14 + 150 + 3 + (100 if dtype == BF else 5) + 3 + 2


def test_seed_slot_resolves_to_the_same_mask():
    a = G.case(63, 83, 128, BF, "drop_res", seed=2 ** 40 + 5)
    b = G.case(63, 83, 128, BF, "drop_res", seed=2 ** 40 + 5, slot=True)
    assert b.seed >> 63 and torch.equal(G.keep_mask(a), G.keep_mask(b))
    assert not torch.equal(G.keep_mask(a), G.keep_mask(G.case(63, 83, 128, BF, "drop_res", seed=2 ** 40 + 6)))


def test_ulp_out():
    x = torch.tensor([1.0, 1.5, 2.0, 3.0, 0.75, 0.0], dtype=torch.float64)
    assert G.ulp_out(x, BF)[:5].tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8]
    assert G.ulp_out(x, FP)[0].item() == 2.0 ** -23 and G.ulp_out(x, FP)[5].item() == 2.0 ** -149
    assert math.isinf(G.judge(torch.tensor([float("nan")], dtype=torch.float64), x[:1], x[:1], x[:1], 8, FP)[3])
