"""st5_relpos_bwd / st5_relpos_dpe_final (csrc/relpos_bwd.hip) against the launch sequence they replace in the fused attention
backward, through the C ABI, on copies of the same seeded operands:

    st5_gemm NT, beta = 1          dQ += alpha * dQP . PE                  (B operand: the K-major copy PE^T, as the call site passes it)
    st5_gemm k-strided, OUT_F32    part[bh] = alpha * dQP[bh]^T . Q[bh]
    st5_colsum_ws (overwrite)      sum over (batch, head), fixed order
    st5_cast_from_f32              fp32 -> bf16

Every comparison is BYTE equality: there is no tolerance.  q / dq are column slices of [B*T (+ 64 guard rows), 3*H*64] buffers as at the call
site; the guard rows behind the last valid row (and 64 behind dQP's) hold 0xFF bytes -- NaN as bf16 -- so a row >= T read into a sum
shows as NaN and a row >= T written shows as a changed byte.  Everything outside the dq slice (the k / v thirds of the gradient buffer)
is compared as well.

Shapes (B, H, T, nb): the smallest at which a tile edge, a reduction tail or a change of the final sum's nsplit can go wrong --
T = 70 (no multiple of 64 or 16; two query tiles, the second with 6 valid rows), 499 (eight tiles), 130 with nb = 128 (one LDS panel, the
smallest nb the NT fast path takes), 96 and 192 (batch, head) rows (nsplit 2 and 3), T = 16 (a single k-chunk)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from speecht5_amd import functional as Fn, hip  # noqa: E402

HD = 64
ALPHA = HD ** -0.5
SHAPES = [(1, 2, 70, 320), (1, 2, 499, 320), (2, 1, 130, 128), (8, 12, 70, 320), (16, 12, 70, 320), (1, 1, 16, 320)]
GUARD = 64
PART_FILL = 0x5A


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b, what):
    a, b = _bytes(a), _bytes(b)
    if not torch.equal(a, b):
        raise AssertionError(f"{what}: {int((a != b).sum())} of {a.numel()} bytes differ")


def _operands(dev, B, H, T, nb):
    """Seeded operands with NaN guard rows: dqp [(B*H*T + 64), nb], qkv / dqkv [(B*T + 64), 3*H*64], pe [nb, 64]."""
    g = torch.Generator().manual_seed(1000 * T + 10 * nb + B * H)
    ld = 3 * H * HD
    dqp = torch.empty(B * H * T + GUARD, nb, dtype=torch.bfloat16)
    dqp[:B * H * T] = (torch.randn(B * H * T, nb, generator=g) * 0.5).to(torch.bfloat16)
    qkv = torch.empty(B * T + GUARD, ld, dtype=torch.bfloat16)
    qkv[:B * T] = (torch.randn(B * T, ld, generator=g) * 1.2).to(torch.bfloat16)
    dqkv = torch.empty(B * T + GUARD, ld, dtype=torch.bfloat16)
    dqkv[:B * T] = torch.randn(B * T, ld, generator=g).to(torch.bfloat16)
    for t, n in ((dqp, B * H * T), (qkv, B * T), (dqkv, B * T)):
        t[n:].view(torch.uint8).fill_(0xFF)
    pe = torch.randn(nb, HD, generator=g).to(torch.bfloat16)
    return dqp.to(dev), qkv.to(dev), pe.to(dev), dqkv.to(dev)


def _part(dev, B, H, nb):
    return torch.full((B * H * nb * HD * 4,), PART_FILL, dtype=torch.uint8, device=dev).view(torch.float32).view(B * H, nb, HD)


def _present(dqp, qkv, pe, dqkv, B, H, T, nb, want_dpe=True):
    """The launches of functional._flash_bwd's GEMM sequence; dqkv is updated in place.  Returns (part, dpe bf16)."""
    dev = dqp.device
    BH, ld = B * H, 3 * H * HD
    L = hip.lib()
    pe_t = pe.t().contiguous()
    a = hip.operand(dqp, nb, zs0=H * T * nb, zs1=T * nb)
    hip.gemm(a, hip.operand(pe_t, nb), hip.operand(dqkv, ld, zs0=T * ld, zs1=HD), T, HD, nb, hip.BF16, batch=BH, zdiv=H, alpha=ALPHA, beta=1.0)
    part = _part(dev, B, H, nb)
    if not want_dpe:
        return part, None
    hip.gemm(a, hip.operand(qkv, ld, zs0=T * ld, zs1=HD), hip.operand(part, HD, zs0=H * nb * HD, zs1=nb * HD), nb, HD, T, hip.BF16,
             batch=BH, zdiv=H, flags=hip.A_KSTRIDED | hip.B_KSTRIDED | hip.OUT_F32, alpha=ALPHA)
    g = torch.empty(nb, HD, dtype=torch.float32, device=dev)
    ws = torch.empty(L.st5_colsum_ws_bytes(BH, nb * HD), dtype=torch.uint8, device=dev)
    hip.check(L.st5_colsum_ws(part.data_ptr(), g.data_ptr(), ws.data_ptr(), BH, nb * HD, nb * HD, 1.0, 0, hip.F32, hip.stream()), "st5_colsum_ws")
    dpe = torch.empty(nb, HD, dtype=torch.bfloat16, device=dev)
    hip.check(L.st5_cast_from_f32(g.data_ptr(), dpe.data_ptr(), 1, nb * HD, 0, hip.BF16, hip.stream()), "st5_cast_from_f32")
    return part, dpe


def _fused(dqp, qkv, pe, dqkv, B, H, T, nb, want_dpe=True, gate=None):
    """st5_relpos_bwd (+ st5_relpos_dpe_final); dqkv is updated in place.  Returns (part, dpe bf16)."""
    dev = dqp.device
    ld = 3 * H * HD
    L = hip.lib()
    part = _part(dev, B, H, nb)
    gp = gate.data_ptr() if gate is not None else None
    hip.check(L.st5_relpos_bwd(dqp.data_ptr(), qkv.data_ptr(), ld, pe.data_ptr(), dqkv.data_ptr(), ld, part.data_ptr() if want_dpe else None,
                               B, H, T, nb, ALPHA, gp, hip.BF16, hip.stream()), "st5_relpos_bwd")
    if not want_dpe:
        return part, None
    dpe = torch.full((nb, HD), 7.0, dtype=torch.bfloat16, device=dev)
    hip.check(L.st5_relpos_dpe_final(part.data_ptr(), dpe.data_ptr(), B * H, nb * HD, gp, hip.BF16, hip.stream()), "st5_relpos_dpe_final")
    return part, dpe


@functools.lru_cache(maxsize=None)
def _case(dev, B, H, T, nb):
    """Operands and the present sequence's results for one shape, computed once and left unchanged."""
    dqp, qkv, pe, dqkv0 = _operands(dev, B, H, T, nb)
    ref_dqkv = dqkv0.clone()
    ref_part, ref_dpe = _present(dqp, qkv, pe, ref_dqkv, B, H, T, nb)
    torch.cuda.synchronize()
    assert torch.isfinite(ref_dqkv[:B * T].float()).all() and torch.isfinite(ref_part).all() and torch.isfinite(ref_dpe.float()).all()
    assert ref_dpe.float().abs().max().item() > 0 and not torch.equal(ref_dqkv[:B * T, :H * HD], dqkv0[:B * T, :H * HD])
    return dqp, qkv, pe, dqkv0, ref_dqkv, ref_part, ref_dpe


@pytest.mark.parametrize("B,H,T,nb", SHAPES)
def test_both_products_and_final_sum_byte_identical(cuda, B, H, T, nb):
    dqp, qkv, pe, dqkv0, ref_dqkv, ref_part, ref_dpe = _case(cuda, B, H, T, nb)
    qkv_before, dqp_before = qkv.clone(), dqp.clone()
    dqkv = dqkv0.clone()
    part, dpe = _fused(dqp, qkv, pe, dqkv, B, H, T, nb)
    torch.cuda.synchronize()
    _same(dqkv, ref_dqkv, "dq slice, k / v thirds and guard rows")
    _same(part, ref_part, "fp32 partials")
    _same(dpe, ref_dpe, "dPE")
    _same(qkv, qkv_before, "q (input)")
    _same(dqp, dqp_before, "dqp (input)")


@pytest.mark.parametrize("B,H,T,nb", [(1, 2, 70, 320), (2, 1, 130, 128)])
def test_dq_half_alone_leaves_part_untouched(cuda, B, H, T, nb):
    dqp, qkv, pe, dqkv0, ref_dqkv, _, _ = _case(cuda, B, H, T, nb)
    dqkv = dqkv0.clone()
    part, _ = _fused(dqp, qkv, pe, dqkv, B, H, T, nb, want_dpe=False)
    torch.cuda.synchronize()
    _same(dqkv, ref_dqkv, "dq slice")
    assert bool((_bytes(part) == PART_FILL).all()), "the workspace was written without being asked for"


def test_guard_rows_unchanged_and_unread(cuda):
    """Rows >= T: the 64 rows of 0xFF bytes behind dq's last valid row keep their bytes, those behind q's and dqp's never reach a sum (NaN)."""
    B, H, T, nb = 1, 2, 70, 320
    dqp, qkv, pe, dqkv0, _, _, _ = _case(cuda, B, H, T, nb)
    dqkv = dqkv0.clone()
    part, dpe = _fused(dqp, qkv, pe, dqkv, B, H, T, nb)
    torch.cuda.synchronize()
    assert bool((_bytes(dqkv[B * T:]) == 0xFF).all()), "a row >= T of dq was written"
    assert bool((_bytes(qkv[B * T:]) == 0xFF).all())
    assert torch.isfinite(part).all() and torch.isfinite(dpe.float()).all() and torch.isfinite(dqkv[:B * T].float()).all(), "a row >= T was read into a sum"


@pytest.mark.parametrize("B,H,T,nb", [(1, 2, 70, 320), (8, 12, 70, 320)])
def test_gate(cuda, B, H, T, nb):
    dqp, qkv, pe, dqkv0, ref_dqkv, ref_part, ref_dpe = _case(cuda, B, H, T, nb)
    keep = torch.ones(1, dtype=torch.float32, device=cuda)
    dqkv = dqkv0.clone()
    part, dpe = _fused(dqp, qkv, pe, dqkv, B, H, T, nb, gate=keep)
    torch.cuda.synchronize()
    _same(dqkv, ref_dqkv, "keep = 1: dq")
    _same(part, ref_part, "keep = 1: partials")
    _same(dpe, ref_dpe, "keep = 1: dPE")
    keep.zero_()
    dqkv = dqkv0.clone()
    part, dpe = _fused(dqp, qkv, pe, dqkv, B, H, T, nb, gate=keep)
    torch.cuda.synchronize()
    _same(dqkv, dqkv0, "keep = 0: dq is left as it was")
    assert bool((_bytes(part) == PART_FILL).all()), "keep = 0: the partials were written"
    assert bool((_bytes(dpe) == 0).all()), "keep = 0: dPE is not exact zeros"


def test_two_launches_identical(cuda):
    B, H, T, nb = 8, 12, 70, 320
    dqp, qkv, pe, dqkv0, _, _, _ = _case(cuda, B, H, T, nb)
    out = []
    for _ in range(2):
        dqkv = dqkv0.clone()
        part, dpe = _fused(dqp, qkv, pe, dqkv, B, H, T, nb)
        torch.cuda.synchronize()
        out.append((dqkv, part, dpe))
    for a, b, what in zip(out[0], out[1], ("dq", "partials", "dPE")):
        _same(a, b, what)


def test_autograd_switch_on_and_off_identical(cuda):
    """Fn.SelfAttentionFunction forward + backward with the one-pass kernel and with the GEMM sequence: same dqkv and dpe bytes."""
    B, H, T, maxrel, pdrop = 2, 2, 70, 160, 0.1
    d = H * HD
    dt = torch.bfloat16
    was = Fn._RELPOS.fused
    Fn.set_compute_dtype(dt)
    g = torch.Generator().manual_seed(5)
    x0 = (torch.randn(B * T, 3 * d, generator=g) * 1.2).to(dt).to(cuda)
    pe0 = torch.randn(2 * maxrel, HD, generator=g).to(dt).to(cuda)
    dout = torch.randn(B * T, d, generator=g).to(dt).to(cuda)
    res = {}
    try:
        for fused in (True, False):
            Fn.set_relpos_bwd_fused(fused)
            assert Fn.relpos_bwd_fused(2 * maxrel) == fused
            Fn.manual_seed(77)
            x = x0.clone().requires_grad_(True)
            pe = pe0.clone().requires_grad_(True)
            pe_t = None if fused else pe0.t().contiguous()      # (what modules/multihead_attention.py passes)
            out = Fn.SelfAttentionFunction.apply(x, pe, None, (B, H, T, HD, maxrel, False, pdrop, pe_t))
            out.backward(dout)
            torch.cuda.synchronize()
            res[fused] = (out.detach().clone(), x.grad.clone(), pe.grad.clone())
    finally:
        Fn.set_relpos_bwd_fused(was)
        Fn.set_compute_dtype(torch.float32)
    assert res[True][2].dtype == dt and res[True][2].float().abs().max().item() > 0
    for a, b, what in zip(res[True], res[False], ("ctx", "dqkv", "dpe")):
        _same(a, b, what)
