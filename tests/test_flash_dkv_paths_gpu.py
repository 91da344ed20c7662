"""The dK/dV backward's path combinations that test_flash_gpu.py::test_second_generation_kernels_bit_identical_to_first leaves out,
in the same style: csrc/flash_attn2.hip (st5_flash_attn_set_impl(2)) against the first-generation kernels of csrc/flash_attn.hip
(impl 1) on identical inputs and dropout seeds, torch.equal on the output and on every gradient (pe.grad = the bucket gradients the
dkv kernel stores through its buffer descriptor, included).  Equality is exact: there is no tolerance.

What the cases reach in fa2::bwd_dkv_kernel:
  * relative bias WITH dropout at T = 700 (maxrel 160): fully clipped, mixed and interior (query sub-tile, key sub-tile) pairs in one
    launch -- the interior store form (scalar offsets), the edge form (out-of-range offsets dropped by the hardware) and no stores;
  * T = 150 and T = 65 with maxrel 16 and key padding: the query tail (rows >= T) and the key tail (keys >= S) inside mixed sub-tiles,
    masked keys (the SLOW select) beside dropout's shared pair hashes;
  * B * H a multiple of 8 (the XCD-aware block_coords map) and not;
  * the two benched encoder shapes (B 16, H 12, T 512 and B 8, H 12, T 499, dropout 0.1) once;
  * cross attention with S != T and causal self-attention, both with dropout (the no-bias kernel's pair hashes, the causal bound)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from speecht5_amd import functional as Fn, hip  # noqa: E402

#        B  H   T    S  causal rel pad pdrop maxrel
CASES = [(2, 3, 700, 700, 0, 1, 0, 0.1, 160),
         (2, 4, 700, 700, 0, 1, 1, 0.1, 160),
         (2, 3, 150, 150, 0, 1, 1, 0.1, 16),
         (2, 4, 150, 150, 0, 1, 1, 0.1, 16),
         (2, 3, 65, 65, 0, 1, 1, 0.1, 16),
         (2, 4, 65, 65, 0, 1, 1, 0.1, 16),
         (16, 12, 512, 512, 0, 1, 1, 0.1, 160),
         (8, 12, 499, 499, 0, 1, 1, 0.1, 160),
         (2, 4, 130, 200, 0, 0, 0, 0.1, 0),
         (2, 3, 200, 77, 0, 0, 1, 0.1, 0),
         (2, 4, 313, 313, 1, 0, 0, 0.1, 0),
         (2, 3, 313, 313, 1, 0, 1, 0.1, 0)]


@pytest.mark.parametrize("B,H,T,S,causal,rel,pad,pdrop,maxrel", CASES)
def test_dkv_paths_bit_identical_to_first_generation(cuda, B, H, T, S, causal, rel, pad, pdrop, maxrel):
    torch.manual_seed(T * 11 + S + H)
    hd = 64
    d = H * hd
    dt = torch.bfloat16
    Fn.set_compute_dtype(dt)
    kpm = torch.zeros(B, S, dtype=torch.uint8)
    if pad:
        for b in range(1, B, 2):                      # odd batch rows end in 3 .. 42 padded keys (different lengths)
            kpm[b, S - (3 + 13 * b) % 40 - 3:] = 1
    KP = kpm.to(cuda) if pad else None
    pe0 = torch.randn(2 * maxrel, hd).to(dt).to(cuda) if rel else None
    dout = torch.randn(B * T, d).to(dt).to(cuda)
    res = {}
    L = hip.lib()
    try:
        for impl in (1, 2):
            hip.check(L.st5_flash_attn_set_impl(impl), "set_impl")
            Fn.manual_seed(91)
            pe = pe0.clone().requires_grad_(True) if rel else None
            if T == S:
                x = (torch.randn(B * T, 3 * d, generator=torch.Generator().manual_seed(1)) * 1.2).to(dt).to(cuda).requires_grad_(True)
                out = Fn.SelfAttentionFunction.apply(x, pe, KP, (B, H, T, hd, maxrel if rel else 0, bool(causal), pdrop))
                out.backward(dout)
                res[impl] = (out.detach().clone(), x.grad.clone(), pe.grad.clone() if rel else None)
            else:
                g = torch.Generator().manual_seed(2)
                xq = (torch.randn(B * T, d, generator=g) * 1.2).to(dt).to(cuda).requires_grad_(True)
                xkv = (torch.randn(B * S, 2 * d, generator=g) * 1.2).to(dt).to(cuda).requires_grad_(True)
                out, _ = Fn.CrossAttentionFunction.apply(xq, xkv, KP, (B, H, T, S, hd, pdrop, False))
                out.backward(dout)
                res[impl] = (out.detach().clone(), xq.grad.clone(), xkv.grad.clone())
            torch.cuda.synchronize()
    finally:
        hip.check(L.st5_flash_attn_set_impl(2), "set_impl")
        Fn.set_compute_dtype(torch.float32)
    for i, name in enumerate(("out", "grad0", "grad1")):
        a, b = res[1][i], res[2][i]
        if a is None:
            continue
        assert torch.isfinite(b.float()).all(), name
        assert b.float().abs().max().item() > 0, name
        if not torch.equal(a, b):
            diff = (a.float() - b.float()).abs()
            raise AssertionError(f"{name}: {int((diff > 0).sum())} of {diff.numel()} elements differ, max {diff.max().item():.3e} "
                                 f"(scale {a.float().abs().max().item():.3e})")
