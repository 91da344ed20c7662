"""CPU pins of tests/attention_reference.py: the fp64 attention reference against torch autograd in fp64, the vectorised dropout
RNG against a scalar line-by-line transcription of csrc/common.h, and the keep fraction of the RNG."""
import math

import numpy as np
import pytest
import torch

from tests import attention_reference as R

M32, M64 = (1 << 32) - 1, (1 << 64) - 1


# ---- scalar transcription of common.h (Python ints, explicit wrap-around) ------------------------------------------------
def s_umul24(a, b):
    return ((a & 0xFFFFFF) * (b & 0xFFFFFF)) & M32


def s_rng_hash64(seed, group):
    z = (group + seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def s_drop_seed_fold(seed):
    h = s_rng_hash64(seed, 0)
    return (h & M32) ^ (h >> 32)


def s_drop_block_key_folded(seed_fold, block):
    x = (block & M32) ^ seed_fold ^ s_umul24(block >> 32, 0x9E3779)
    x ^= x >> 15; x = s_umul24(x, 0x9E3779)
    x ^= x >> 12; x = s_umul24(x, 0x85EBCB)
    x ^= x >> 15
    return x


def s_drop_pair_bits(key, pair):
    x = key ^ ((pair * 0x9E3779B1) & M32)
    x ^= x >> 16; x = s_umul24(x, 0xCA6B85)
    x ^= x >> 13; x = s_umul24(x, 0xB2AE35)
    x ^= x >> 16
    return x


def s_keep(seed, idx, p):
    thresh = int(np.float32(p) * np.float32(65536.0))
    key = s_drop_block_key_folded(s_drop_seed_fold(seed), idx >> 6)
    bits = s_drop_pair_bits(key, (idx & 63) >> 1)
    return ((bits >> 16) if (idx & 1) else (bits & 0xFFFF)) >= thresh


@pytest.mark.parametrize("seed", [0, 1, 4242, 0x7FFF_FFFF_FFFF_FFFF, 0x1234_5678_9ABC_DEF0])
def test_rng_matches_scalar_transcription(seed):
    rng = np.random.default_rng(seed & 0xFFFF)
    idx = np.concatenate([np.arange(0, 700), rng.integers(0, 1 << 40, 1500), (1 << 32) - 300 + np.arange(600),
                          rng.integers(1 << 32, 1 << 62, 1000)]).astype(np.uint64)
    for p in (0.1, 0.5, 0.05):
        got = R.keep_mask_flat(seed, p, idx)
        want = np.array([s_keep(seed, int(i), p) for i in idx])
        assert np.array_equal(got, want), (seed, p, np.flatnonzero(got != want)[:5])
    # the pieces one by one (block keys at blocks >= 2^32, where block >> 32 enters through __umul24)
    blocks = (idx >> np.uint64(6))
    sf = s_drop_seed_fold(seed)
    assert int(R.drop_seed_fold(seed)) == sf
    assert (blocks >> np.uint64(32)).max() > 0
    assert [int(x) for x in R.drop_block_key_folded(sf, blocks)] == [s_drop_block_key_folded(sf, int(b)) for b in blocks]


def test_attention_layout_is_the_flat_rng_at_row_stride():
    BH, T, S, seed, p = 3, 5, 100, 99, 0.1
    m = R.keep_mask_attention(seed, p, BH, T, S)
    assert R.attention_row_stride(100) == 128 and R.attention_row_stride(64) == 64 and R.attention_row_stride(1) == 64
    for bh in range(BH):
        for i in range(T):
            want = [s_keep(seed, (bh * T + i) * 128 + j, p) for j in range(S)]
            assert m[bh, i].tolist() == want
    assert np.array_equal(R.keep_mask_attention(seed, p, BH, T, S, rows=[2, 0]), m[[2, 0]])


def test_threshold_and_keep_scale_in_float32():
    # float32(0.1) * 65536 = 6553.6000976... -> 6553; float32 1 / (1 - 0.1f) = 1.1111112
    assert R.dropout_thresh(0.1) == 6553 and R.dropout_thresh(0.5) == 32768 and R.dropout_thresh(0.0) == 0
    assert R.inv_keep(0.1) == float(np.float32(1) / np.float32(0.9))
    assert R.inv_keep(0.1) != 1 / 0.9


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_fraction(p):
    n = 1_000_000
    keep = R.keep_mask_flat(12345, p, np.arange(n, dtype=np.uint64) + np.uint64(7 << 32))
    q = 1 - R.dropout_thresh(p) / 65536.0
    sigma = math.sqrt(q * (1 - q) / n)
    assert abs(keep.mean() - (1 - p)) <= 5 * sigma, (keep.mean(), 1 - p, sigma)


# ---- fp64 reference vs torch autograd -----------------------------------------------------------------------------------
def _autograd(q, k, v, dout, pe, maxrel, kpm, causal, keep, p, dprobs=None):
    q, k, v = (x.clone().requires_grad_(True) for x in (q, k, v))
    pe = pe.clone().requires_grad_(True) if pe is not None else None
    B, H, T, hd = q.shape
    S = k.shape[2]
    scale = hd ** -0.5
    s = torch.einsum("bhid,bhjd->bhij", q * scale, k)
    if pe is not None:
        s = s + torch.einsum("bhid,ijd->bhij", q * scale, pe[R.buckets(T, S, maxrel)])
    vis = torch.stack([R.visible(T, S, None if kpm is None else kpm[b], causal) for b in range(B)])[:, None]
    s = s.masked_fill(~vis, -math.inf)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None].masked_fill(~vis.any(-1, keepdim=True), 0.0)).masked_fill(~vis, 0.0)
    Pd = P * torch.as_tensor(keep).reshape(B, H, T, S).double() * R.inv_keep(p) if keep is not None else P
    o = Pd @ v
    loss = (o * dout).sum() + ((P * dprobs).sum() if dprobs is not None else 0.0)
    loss.backward()
    return dict(o=o.detach(), lse=lse.detach().masked_fill(~vis.any(-1), math.inf), probs=P.detach() if dprobs is not None else None,
                dq=q.grad, dk=k.grad, dv=v.grad, dpe=None if pe is None else pe.grad)


CASES = [  # B, H, T, S, rel, causal, pad, drop
    (2, 2, 17, 17, 1, 0, 0, 0), (2, 3, 70, 70, 1, 0, 1, 1), (1, 2, 40, 40, 1, 1, 1, 1), (2, 2, 33, 33, 0, 1, 0, 0),
    (2, 2, 50, 9, 0, 0, 1, 1), (2, 1, 5, 70, 0, 0, 1, 0), (1, 2, 1, 1, 1, 1, 0, 0), (2, 2, 64, 64, 1, 0, 2, 1),
    (2, 2, 30, 12, 0, 0, 1, 2),   # drop == 2: dropout and a gradient on the probabilities (the guided-attention loss)
]


@pytest.mark.parametrize("B,H,T,S,rel,causal,pad,drop", CASES)
def test_fp64_reference_matches_autograd(B, H, T, S, rel, causal, pad, drop):
    g = torch.Generator().manual_seed(T * 100 + S)
    hd, maxrel = 16, 6
    q, dout = (torch.randn(B, H, T, hd, generator=g, dtype=torch.float64) for _ in range(2))
    k, v = (torch.randn(B, H, S, hd, generator=g, dtype=torch.float64) for _ in range(2))
    pe = torch.randn(2 * maxrel, hd, generator=g, dtype=torch.float64) if rel else None
    kpm = None
    if pad:
        kpm = torch.zeros(B, S, dtype=torch.uint8)
        kpm[-1, S - 3:] = 1
        if pad == 2:
            kpm[-1, :] = 1            # every key of the last item padded: O = 0, LSE = +inf, zero gradients
    p = 0.3 if drop else 0.0
    keep = R.keep_mask_attention(7, p, B * H, T, S).astype(np.float64) if drop else None
    dprobs = torch.randn(B, H, T, S, generator=g, dtype=torch.float64) if drop == 2 else None
    got = R.attention_fwd_bwd_fp64(q, k, v, dout, pe, maxrel, kpm, bool(causal), keep, p, dprobs)
    ref = _autograd(q, k, v, dout, pe, maxrel, kpm, bool(causal), keep, p, dprobs)
    for nm in ("o", "lse", "probs", "dq", "dk", "dv", "dpe"):
        if ref[nm] is None:
            assert got[nm] is None
            continue
        a, b = got[nm], ref[nm].nan_to_num(0.0) if nm != "lse" else ref[nm]
        fin = torch.isfinite(b)
        assert torch.equal(torch.isfinite(a), fin), nm
        assert (a[fin] - b[fin]).abs().max().item() <= 1e-12 * max(1.0, b[fin].abs().max().item()), nm
    if pad == 2:
        assert torch.all(got["o"][-1] == 0) and torch.all(torch.isinf(got["lse"][-1])) and torch.all(got["dq"][-1] == 0)


def test_emulation_is_close_to_but_not_fp64():
    g = torch.Generator().manual_seed(3)
    B, H, T, S, hd, maxrel = 1, 2, 90, 90, 64, 20
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).double()   # noqa: E731
    q, k, v, dout = bf(B, H, T, hd), bf(B, H, S, hd), bf(B, H, S, hd), bf(B, H, T, hd)
    pe = bf(2 * maxrel, hd)
    keep = R.keep_mask_attention(5, 0.1, B * H, T, S)
    r = R.attention_fwd_bwd_fp64(q, k, v, dout, pe, maxrel, None, False, keep, 0.1)
    e = R.attention_bf16_emulation(q, k, v, dout, pe, maxrel, None, False, keep, 0.1)
    for nm in ("o", "dq", "dk", "dv", "dpe"):
        err = ((e[nm].double() - r[nm]).norm() / r[nm].norm()).item()
        assert 0 < err <= 2 ** -6, (nm, err)
