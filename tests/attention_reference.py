"""Plain references of the attention core, the yardsticks tests/test_attention_fp64_gpu.py holds the fused kernels to:

- attention_fwd_bwd_fp64: forward and backward of one attention call in fp64 (torch, CPU), head by head, in the project's semantics
  (multihead_attention.py + the Shaw bias of encoder.py): bucket = clamp(i - j, -maxrel, maxrel - 1) + maxrel, bias = (q * scale) .
  pe[bucket], causal keys j <= i + (S - T), key padding, dropout O = (P * M / keep) . V with the LSE unaffected by dropout.  Query
  rows with no visible key follow the kernels' convention: O = 0, LSE = +inf, no gradient.
- attention_bf16_emulation: the same in fp32 torch, rounding to bf16 where the second-generation kernels (csrc/flash_attn2.hip) do;
  its error against fp64 is the bar the kernels are judged by.
- the dropout counter RNG of csrc/common.h (rng_hash64 -> drop_seed_fold -> drop_block_key_folded -> drop_pair_bits -> drop_keep)
  restated in vectorised numpy, with the flat counter layout of st5_dropout (idx) and the attention layout of the softmax and both
  flash generations (idx = (bh * T + i) * round_up(ceil8(S), 64) + j, drop_row_stride).

tests/test_attention_reference_cpu.py pins the fp64 reference to torch autograd and the RNG to a scalar transcription of common.h."""
import math

import numpy as np
import torch

LOG2E = 1.4426950408889634
M32 = np.uint64(0xFFFFFFFF)
M24 = np.uint64(0xFFFFFF)


# ---------------------------------------------------------------------------------------------------------------------------
# dropout counter RNG (common.h)
# ---------------------------------------------------------------------------------------------------------------------------
def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def umul24(a, b):
    """__umul24: product of the low 24 bits of both operands, low 32 bits of the result."""
    return ((_u64(a) & M24) * (_u64(b) & M24)) & M32


def rng_hash64(seed, group):
    """splitmix64 finaliser of seed * golden + group (mod 2^64)."""
    with np.errstate(over="ignore"):
        z = _u64(group) + _u64(seed) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x632BE59BD9B4E019)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def drop_seed_fold(seed):
    """Seed part of the block keys (seeds below 2^63: bit 63 marks a device slot, not restated here)."""
    assert 0 <= int(seed) < 2 ** 63
    h = rng_hash64(np.uint64(seed), np.uint64(0))
    return (h & M32) ^ (h >> np.uint64(32))


def drop_block_key_folded(seed_fold, block):
    block = _u64(block)
    x = (block & M32) ^ _u64(seed_fold) ^ umul24(block >> np.uint64(32), 0x9E3779)
    x ^= x >> np.uint64(15)
    x = umul24(x, 0x9E3779)
    x ^= x >> np.uint64(12)
    x = umul24(x, 0x85EBCB)
    x ^= x >> np.uint64(15)
    return x


def drop_pair_bits(key, pair):
    x = _u64(key) ^ ((_u64(pair) * np.uint64(0x9E3779B1)) & M32)
    x ^= x >> np.uint64(16)
    x = umul24(x, 0xCA6B85)
    x ^= x >> np.uint64(13)
    x = umul24(x, 0xB2AE35)
    x ^= x >> np.uint64(16)
    return x


def drop_keep(bits, odd, thresh16):
    bits = _u64(bits)
    half = np.where(np.asarray(odd, dtype=bool), bits >> np.uint64(16), bits & np.uint64(0xFFFF))
    return half >= np.uint64(thresh16)


def dropout_thresh(p):
    """(unsigned)(p * 65536.0f), evaluated in float32 as the kernels do."""
    return int(np.float32(p) * np.float32(65536.0))


def inv_keep(p):
    """1 / (1 - p) in float32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask_flat(seed, p, idx):
    """Keep (True) / drop of the elements with counters `idx` (uint64 array, any shape)."""
    idx = _u64(idx)
    key = drop_block_key_folded(drop_seed_fold(seed), idx >> np.uint64(6))
    bits = drop_pair_bits(key, (idx & np.uint64(63)) >> np.uint64(1))
    return drop_keep(bits, (idx & np.uint64(1)).astype(bool), dropout_thresh(p))


def attention_row_stride(S):
    """drop_row_stride(ceil8(S)): the counter stride of one query row of attention probabilities."""
    lds = (S + 7) // 8 * 8
    return (lds + 63) // 64 * 64


def draws_attention(seed, BH, T, S, rows=None):
    """The 16-bit draws [BH, T, S] (uint64) of attention probabilities, idx = (bh * T + i) * round_up(ceil8(S), 64) + j; an
    element is kept <=> draw >= dropout_thresh(p).  rows: optional subset of bh to evaluate (returns [len(rows), T, S])."""
    bhs = np.arange(BH, dtype=np.uint64) if rows is None else _u64(rows)
    R = np.uint64(attention_row_stride(S))
    # one block key per 64-key block of each row, then the pair hashes of the row's S keys
    nblk = (S + 63) // 64
    row = (bhs[:, None] * np.uint64(T) + np.arange(T, dtype=np.uint64)[None, :])            # [n, T]
    blocks = row[:, :, None] * (R >> np.uint64(6)) + np.arange(nblk, dtype=np.uint64)        # [n, T, nblk]
    keys = drop_block_key_folded(drop_seed_fold(seed), blocks)
    j = np.arange(S, dtype=np.uint64)
    bits = drop_pair_bits(keys[:, :, (j >> np.uint64(6)).astype(np.int64)], (j & np.uint64(63)) >> np.uint64(1))
    return np.where((j & np.uint64(1)).astype(bool), bits >> np.uint64(16), bits & np.uint64(0xFFFF))


def keep_mask_attention(seed, p, BH, T, S, rows=None):
    """Keep mask [BH, T, S] (bool) of attention probabilities (draws_attention >= dropout_thresh(p))."""
    return draws_attention(seed, BH, T, S, rows) >= np.uint64(dropout_thresh(p))


# ---------------------------------------------------------------------------------------------------------------------------
# attention core
# ---------------------------------------------------------------------------------------------------------------------------
def buckets(T, S, maxrel):
    i = torch.arange(T)[:, None]
    j = torch.arange(S)[None, :]
    return (i - j).clamp(-maxrel, maxrel - 1) + maxrel


def visible(T, S, kpm_b, causal):
    """[T, S] bool: key j is visible from query i (not padded, and j <= i + (S - T) when causal)."""
    vis = torch.ones(T, S, dtype=torch.bool)
    if causal:
        vis = torch.ones(T, S, dtype=torch.bool).tril(S - T)
    if kpm_b is not None:
        vis = vis & ~kpm_b.bool()[None, :]
    return vis


def _as(x, dtype):
    return None if x is None else x.detach().cpu().to(dtype)


def attention_fwd_bwd_fp64(q, k, v, dout, pe=None, maxrel=0, kpm=None, causal=False, keep=None, p=0.0, dprobs=None):
    """q [B,H,T,hd], k / v [B,H,S,hd], dout [B,H,T,hd], pe [2*maxrel, hd] or None, kpm [B,S] (nonzero = padded) or None,
    keep: the dropout mask, [B*H, T, S] (0 / 1, numpy or torch) or a function bh -> [T, S], or None; p the dropout rate it was
    drawn with; dprobs [B,H,T,S] or None: a gradient that reaches the (undropped) probabilities directly (guided attention).
    Returns dict(o, lse [B,H,T] (natural log; +inf for rows without a visible key), probs [B,H,T,S] (with dprobs, else None),
    dq, dk, dv, dpe (or None), rho = dict(dq [B,H,T], dk [B,H,S], dpe [nb] or None): per row, a bound on how far rounding O to bf16
    before D = dO . O (as the kernels do) moves that gradient row -- dS_ij moves by -P_ij dD_i with |dD_i| <= 2^-8 sum |dO_i| |O_i|),
    all fp64."""
    return _attention(q, k, v, dout, pe, maxrel, kpm, causal, keep, p, dprobs, emulate=False)


def attention_bf16_emulation(q, k, v, dout, pe=None, maxrel=0, kpm=None, causal=False, keep=None, p=0.0):
    """fp32 restatement of the second-generation fused kernels (csrc/flash_attn2.hip) on the same bf16 inputs, rounding to bf16
    where they do:
      * the relative-position table QP = bf16(scale * log2(e) * q . pe^T) (qp_table_kernel), scores s * scale * log2(e) + QP[bucket]
        in the log2 domain;
      * P = exp2(x - m) in bf16 before P . V (pack8 in fwd_kernel; unnormalised, kept elements only, 1/keep and 1/l applied to O);
      * D = dO . O from the bf16 O the forward wrote (dvec);
      * dS = P * (dP * M / keep - D) in bf16 before dQ and dK (bwd_dq_kernel, bwd_dkv_kernel);
      * P * M / keep in bf16 before dV (bwd_dkv_kernel);
      * dQP in bf16 (interior buckets stored per element, the clipped end buckets summed in fp32 first), then
        dQ += scale * dQP . PE and dPE = scale * sum_bh dQP^T . Q as fp32 products of the bf16 operands;
      * O, dQ, dK, dV in bf16 (dQ rounded once after the kernel and once after the dQP product).
    The online softmax's per-tile rescaling is not restated (P is taken against the row maximum)."""
    return _attention(q, k, v, dout, pe, maxrel, kpm, causal, keep, p, None, emulate=True)


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _attention(q, k, v, dout, pe, maxrel, kpm, causal, keep, p, dprobs, emulate):
    dt = torch.float32 if emulate else torch.float64
    rnd = _bf if emulate else (lambda x: x)
    q, k, v, dout, pe = (_as(x, dt) for x in (q, k, v, dout, pe))
    B, H, T, hd = q.shape
    S = k.shape[2]
    scale = hd ** -0.5
    ik = inv_keep(p) if (keep is not None and p > 0) else 1.0
    if keep is not None and not callable(keep):
        keep = torch.as_tensor(np.asarray(keep)).reshape(B * H, T, S)
    bk = buckets(T, S, maxrel) if pe is not None else None
    nb = pe.shape[0] if pe is not None else 0
    o = torch.zeros(B, H, T, hd, dtype=dt)
    lse = torch.full((B, H, T), math.inf, dtype=torch.float64)
    probs = torch.zeros(B, H, T, S, dtype=dt) if dprobs is not None else None
    dq = torch.zeros(B, H, T, hd, dtype=dt)
    dk = torch.zeros(B, H, S, hd, dtype=dt)
    dv = torch.zeros(B, H, S, hd, dtype=dt)
    dpe = torch.zeros(nb, hd, dtype=dt) if pe is not None else None
    # sensitivity of dQ / dK / dPE rows to rounding O to bf16 before D = dO . O (only the fp64 reference fills it)
    rho = None if emulate else dict(dq=torch.zeros(B, H, T), dk=torch.zeros(B, H, S), dpe=torch.zeros(nb) if pe is not None else None)
    for b in range(B):
        vis = visible(T, S, None if kpm is None else kpm[b].cpu(), causal)
        live = vis.any(1)                                                   # rows with at least one visible key
        for h in range(H):
            qh, kh, vh, gh = q[b, h], k[b, h], v[b, h], dout[b, h]
            M = None
            if keep is not None:
                M = torch.as_tensor(np.asarray(keep(b * H + h) if callable(keep) else keep[b * H + h])).to(dt)
            if emulate:   # log2 domain, bias table in bf16
                x = (qh @ kh.t()) * (scale * LOG2E)
                if pe is not None:
                    qp = _bf((qh @ pe.t()) * (scale * LOG2E))
                    x = x + torch.gather(qp, 1, bk)
            else:
                x = (qh * scale) @ kh.t()
                if pe is not None:
                    x = x + torch.gather((qh * scale) @ pe.t(), 1, bk)
            x = x.masked_fill(~vis, -math.inf)
            m = x.max(1, keepdim=True).values
            m = torch.where(live[:, None], m, torch.zeros_like(m))
            e = (torch.exp2(x - m) if emulate else torch.exp(x - m)).masked_fill(~vis, 0.0)
            l = e.sum(1, keepdim=True)
            linv = torch.where(live[:, None], 1.0 / l.clamp_min(1e-300 if not emulate else 1e-38), torch.zeros_like(l))
            em = e * M if M is not None else e
            oh = (rnd(em) @ vh) * (linv * ik)
            oh = rnd(oh)
            o[b, h] = oh
            ls = (m * math.log(2.0) + torch.log(l)).double() if emulate else m + torch.log(l)   # (fp32 in the kernels)
            lse[b, h] = torch.where(live, ls[:, 0], torch.full_like(ls[:, 0], math.inf))
            # backward: P recomputed against the LSE (kernels: exp2(x - lse * log2 e)); rows without a visible key have P = 0
            P = e * linv
            D = (gh * oh).sum(1, keepdim=True)
            if rho is not None:
                # |dO . (O - bf16(O))| <= 2^-9 sum |dO| |O|, taken twice; it moves dS_ij by -P_ij dD_i
                dD = 2.0 ** -8 * (gh.abs() * oh.abs()).sum(1)
                pk = P @ kh
                if pe is not None:
                    Pb = torch.zeros(T, nb, dtype=dt).scatter_add_(1, bk, P)
                    pk = pk + Pb @ pe
                    rho["dpe"] += scale * (Pb * dD[:, None]).t() @ qh.norm(dim=1)
                rho["dq"][b, h] = scale * dD * pk.norm(dim=1)
                rho["dk"][b, h] = scale * (P * dD[:, None]).t() @ qh.norm(dim=1)
            dP = gh @ vh.t()
            dPd = dP * M * ik if M is not None else dP
            dS = P * (dPd - D)
            if dprobs is not None:
                G = _as(dprobs[b, h], dt)
                dS = dS + P * (G - (P * G).sum(1, keepdim=True))
            if probs is not None:
                probs[b, h] = P
            Pd = P * M * ik if M is not None else P
            dv[b, h] = rnd(rnd(Pd).t() @ gh)
            dSr = rnd(dS)
            dqh = rnd((dSr @ kh) * scale)
            dk[b, h] = rnd((dSr.t() @ qh) * scale)
            if pe is not None:
                dqp = torch.zeros(T, nb, dtype=dt).scatter_add_(1, bk, dS)   # end buckets: fp32 sums of dS, then one rounding
                dqp = rnd(dqp)
                dqh = rnd(dqh + (dqp @ pe) * scale)
                dpe += (dqp.t() @ qh) * scale
            dq[b, h] = dqh
    return dict(o=o, lse=lse, probs=probs, dq=dq, dk=dk, dv=dv, dpe=dpe, rho=rho)
