"""Plain references of the normalisation family, the yardsticks tests/test_norm_fp64_gpu.py holds csrc/norm.hip, csrc/softmax.hip and
csrc/batchnorm.hip to.  Every operation comes in two forms (one function, `emulate` = False / True):

- fp64: the truth, explicit formulas in torch / numpy double evaluated on the already-rounded inputs;
- emulation: the same arithmetic in fp32 with the kernels' rounding points -- bf16 inputs, outputs rounded to bf16, `dx_dropped` masking
  the ROUNDED dx, dgamma / dbeta in fp32, BatchNorm statistics in fp64 then cast, softmax probabilities rounded before the backward
  reuses them.  The row sums whose rounding a badly conditioned row amplifies (LayerNorm mean, softmax denominators) are taken in the
  kernels' own order (lane_order_sum: a lane's elements serially, then the DPP tree of common.h's wave_sum), so that a one-row case is
  not judged against an emulation that happened to round the other way.  The sums over ROWS (dgamma, dbeta, dQP) are not reproduced.

Also here: the dropout counter layouts these kernels use (flat row * cols + col for LayerNorm's dropped dx and BatchNorm,
rowid * drop_row_stride(lds) + j for the softmax), the case generators both test files share, and the metric and bars
(row_metric, passes).  `fault=` plants one wrong-kernel behaviour in an emulation; tests/test_norm_reference_cpu.py shows that
every one of them fails the bars.  Pinned to torch fp64 autograd by tests/test_norm_reference_cpu.py."""
import math

import numpy as np
import torch

from tests import attention_reference as A

U32 = 2.0 ** -24          # unit roundoff, fp32
U_BF16 = 2.0 ** -9        # unit roundoff, bf16 (8-bit significand, round to nearest)
BAR = 4.0                 # kernel worst row <= BAR x emulation worst row (tests/test_attention_fp64_gpu.py)
EMU_CAP_BF16 = 2.0 ** -6  # the emulation's own worst row with bf16 outputs (same file)
LOG2E_F32 = np.float32(1.4426950408889634)
F32 = np.float32


def unit(dtype):
    return U_BF16 if dtype == torch.bfloat16 else U32


def rnd(x, dtype):
    """Round an fp32 tensor to `dtype` and back."""
    return x.to(dtype).to(torch.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------------------------------------------------------------------
# counters of the dropout RNG (common.h; the hash itself is restated in attention_reference)
# ---------------------------------------------------------------------------------------------------------------------------
def drop_row_stride(row_len):
    """common.h drop_row_stride: the counter stride of one row of `row_len` stored elements, rounded up to 64 (beside
    attention_reference.attention_row_stride(S) = drop_row_stride(ceil8(S)))."""
    return (int(row_len) + 63) // 64 * 64


def keep_mask_rows(seed, p, rows, cols):
    """[rows, cols] bool, counter row * cols + col: LayerNorm's dx_dropped, BatchNorm's dropout."""
    idx = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(cols) + np.arange(cols, dtype=np.uint64)[None, :]
    return A.keep_mask_flat(seed, p, idx)


def keep_mask_softmax(seed, p, nrows, S, lds, stride=None):
    """[nrows, S] bool, counter rowid * drop_row_stride(lds) + j (rowid = bh * T + i)."""
    stride = drop_row_stride(lds) if stride is None else stride
    idx = np.arange(nrows, dtype=np.uint64)[:, None] * np.uint64(stride) + np.arange(S, dtype=np.uint64)[None, :]
    return A.keep_mask_flat(seed, p, idx)


def bucket_table(T, S, maxrel):
    """[T, S] long: clip(i - j, -maxrel, maxrel - 1) + maxrel (softmax.hip bucket())."""
    d = np.arange(T)[:, None] - np.arange(S)[None, :]
    return _t(np.clip(d, -maxrel, maxrel - 1) + maxrel).long()


# ---------------------------------------------------------------------------------------------------------------------------
# row sums in the kernels' order
# ---------------------------------------------------------------------------------------------------------------------------
def lane_order_sum(v, group):
    """Sum over the last axis of v (numpy float32 [R, C]) as a wave does it.  group = 4: lane l owns the 4-element vectors l, l + 64,
    ... (the vector LayerNorm kernels); group = 8: lane l owns elements c * 512 + 8 l .. + 7 of every 512-element chunk c (scalar
    LayerNorm kernels, softmax).  A lane adds its elements serially in index order, then wave_sum: row_shr 1, 2, 4, 8 inside each
    16-lane row, row_bcast 15 into rows 1 and 3, row_bcast 31 into rows 2 and 3, lane 63 read."""
    v = np.asarray(v, dtype=np.float32)
    R, C = v.shape
    per = 64 * group
    n = (C + per - 1) // per
    if n * per != C:
        v = np.concatenate([v, np.zeros((R, n * per - C), dtype=np.float32)], axis=1)
    a = v.reshape(R, n, 64, group)
    s = np.zeros((R, 64), dtype=np.float32)
    for i in range(n):
        for e in range(group):
            s = s + a[:, i, :, e]
    s = s.reshape(R, 4, 16)
    for sh in (1, 2, 4, 8):
        add = np.zeros_like(s)
        add[:, :, sh:] = s[:, :, :-sh]
        s = s + add
    d = s[:, :, 15]
    return (d[:, 3] + d[:, 2]) + (d[:, 1] + d[:, 0])


def _ln_vec(cols):
    return cols % 4 == 0 and cols <= 2048


def _ln_mean_of(s, cols):
    """vector kernels: wave_sum * (1.f / cols); scalar kernels: wave_sum / cols."""
    return s * (F32(1.0) / F32(cols)) if _ln_vec(cols) else s / F32(cols)


def ln_blocks(rows, max_blocks=256):
    """norm.hip ln_blocks: blocks of 16 rows a trip, the same number of trips for every wave once the cap is hit."""
    n = max((rows + 15) // 16, 1)
    if n <= max_blocks:
        return n
    trips = (n + max_blocks - 1) // max_blocks
    return (n + trips - 1) // trips


def ln_trips(rows, max_blocks=256):
    """(fewest, most) trips a wave that has work makes."""
    stride = ln_blocks(rows, max_blocks) * 16
    groups = (rows + 3) // 4
    per = stride // 4
    return max(groups // per, 1), (groups + per - 1) // per


def ln_sum_chain(rows, max_blocks=256):
    """Longest addition chain of a dgamma / dbeta element.  Vector path: a lane's rows (4 per trip) + 4 waves + the block partials
    (16 interleaved serial sums, then 16) + the accumulation; column-reduction path (cols > 2048, cols % 4, dx == NULL): a thread's
    rows + 8 row lanes + the splits (<= 64) + the accumulation.  The larger of the two."""
    nb = ln_blocks(rows, max_blocks)
    vec = 4 * ln_trips(rows, max_blocks)[1] + 4 + (nb + 15) // 16 + 16 + 1
    ns = min(max((rows + 63) // 64, 1), 64)
    col = (rows + ns * 8 - 1) // (ns * 8) + 8 + ns + 1
    return max(vec, col)


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))


def gelu_grad64(z):
    return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327


_GELU_POLY = (-3.086644655e-12, 3.179429497e-10, -1.470189481e-08, 4.085038654e-07, -7.744979484e-06, 1.082136150e-04,
              -1.169087715e-03, 9.949624538e-03, -6.647801399e-02, 3.989412189e-01)
_GELU_GRAD_POLY = (1.668488481e-12, -1.931875215e-10, 1.003747396e-08, -3.115285097e-07, 6.503215900e-06, -9.763300477e-05,
                   1.097474480e-03, -9.375064634e-03, 5.970102549e-02, -2.658985257e-01, 7.978798151e-01)


def _horner32(coef, clamp, z):
    xc = z.clamp(-clamp, clamp)
    v = xc * xc
    h = torch.full_like(z, coef[0])
    for c in coef[1:]:
        h = h * v + c
    return xc * h + 0.5


def gelu32(z, poly):
    """fp32 GELU as the fused LayerNorm kernels evaluate it: erf in fp32 mode, common.h's gelu_poly (Phi = 0.5 + xc G(xc^2)) in bf16 mode."""
    return z * _horner32(_GELU_POLY, 4.242640495300293, z) if poly else 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))


def gelu_grad32(z, poly):
    """common.h gelu_grad_f (fp32 mode) / gelu_grad_poly (bf16 mode)."""
    if poly:
        return _horner32(_GELU_GRAD_POLY, 4.349999904632568, z)
    return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps, dtype=None, emulate=False, gelu=False, keep=1.0, skip=None, fault=None):
    """y, mean, rstd of LayerNorm over the last axis of x [rows, cols]: biased variance, eps inside the root; gelu: y = GELU_erf(LN(x))
    (st5_layernorm_gelu_fwd); keep == 0: y = skip (LayerDrop gate; mean / rstd are written all the same).
    fault: 'prev_row_mean' | 'unbiased_var' | 'skip_last_chunk'."""
    rows, cols = x.shape
    if not emulate:
        xd, g, b = x.double(), gamma.double(), beta.double()
        mean = xd.sum(1) / cols
        d = xd - mean[:, None]
        rstd = 1.0 / torch.sqrt((d * d).sum(1) / cols + float(F32(eps)))
        y = d * rstd[:, None] * g + b
        if gelu:
            y = gelu64(y)
        if keep == 0:
            y = skip.double()
        return y, mean, rstd
    group = 4 if _ln_vec(cols) else 8
    xf = x.float().numpy()
    live = np.ones(cols, dtype=bool)
    if fault == "skip_last_chunk" and cols % (64 * group):
        live[cols // (64 * group) * (64 * group):] = False          # the partially filled last chunk never reaches the row sums
    s = lane_order_sum(xf * live, group)
    mu = _ln_mean_of(s, cols)
    # hipcc contracts `mu = wave_sum(s) * inv_n; d = v - mu` of the vector kernel into one fma (v_fma_f32 d, -inv_n, sum, v:
    # profiles/norm_fp64_isa_excerpts.txt): d is rounded once from v - s * inv_n with the product exact, while the mean that is written
    # out is the rounded product.  Where cols is no power of two, inv_n carries its own rounding (up to 2^-25 relative), and a row with
    # |mean| >> std sees it in every element of y.  (fp64 holds the product of two fp32 exactly.)
    mu_d = s.astype(np.float64) * np.float64(F32(1.0) / F32(cols)) if _ln_vec(cols) else mu.astype(np.float64)
    if fault == "prev_row_mean":
        mu, mu_d = np.concatenate([mu[:1], mu[:-1]]), np.concatenate([mu_d[:1], mu_d[:-1]])
    d = (xf.astype(np.float64) - mu_d[:, None]).astype(np.float32)
    q = lane_order_sum(d * d * live, group)
    var = q / F32(cols - 1) if fault == "unbiased_var" else _ln_mean_of(q, cols)
    rs = (F32(1.0) / np.sqrt(var + F32(eps))).astype(np.float32)
    y = _t(d * rs[:, None]) * gamma.float() + beta.float()
    if gelu:
        y = gelu32(y, dtype == torch.bfloat16)
    if keep == 0:
        y = skip.float()
    return rnd(y, dtype), _t(mu), _t(rs)


def layernorm_bwd(dy, x, gamma, mean, rstd, dtype=None, emulate=False, beta=None, addend=None, keep=1.0, drop=None, dgamma0=None,
                  dbeta0=None, fault=None, max_blocks=256):
    """dx, dgamma, dbeta (accumulated onto dgamma0 / dbeta0), dx_dropped (or None) of the LayerNorm backward.  mean / rstd: the
    forward's (fp64 from layernorm_fwd(emulate=False), fp32 from the emulation).  beta given: the GELU-fused pair, dy is the gradient
    of GELU(LN(x)).  addend: dx += addend (st5_layernorm_bwd_add).  keep == 0: the incoming gradient counts as zero.  drop = (seed, p):
    dx_dropped = round(dx) * mask / (1 - p) with the counter row * cols + col.
    fault: 'trip_tail' (the last 4-row group of the first trip never reaches dgamma / dbeta)."""
    rows, cols = x.shape
    dt = torch.float32 if emulate else torch.float64
    xd, g = x.to(dt), gamma.to(dt)
    mu, rs = mean.to(dt)[:, None], rstd.to(dt)[:, None]
    xh = (xd - mu) * rs
    d = dy.to(dt) * (1.0 if keep != 0 else 0.0)
    if beta is not None:
        z = xh * g + beta.to(dt)
        d = d * (gelu_grad32(z, dtype == torch.bfloat16) if emulate else gelu_grad64(z))
    gg = d * g
    if emulate:
        group = 4 if _ln_vec(cols) else 8
        s1 = _t(_ln_mean_of(lane_order_sum(gg.numpy(), group), cols))[:, None]
        s2 = _t(_ln_mean_of(lane_order_sum((gg * xh).numpy(), group), cols))[:, None]
    else:
        s1, s2 = gg.sum(1, keepdim=True) / cols, (gg * xh).sum(1, keepdim=True) / cols
    dx = rs * (gg - s1 - xh * s2)
    if addend is not None:
        dx = dx + addend.to(dt)
    if emulate:
        dx = rnd(dx, dtype)
    dxd = None
    if drop is not None:
        seed, p = drop
        m = _t(keep_mask_rows(seed, p, rows, cols)).to(dt) * A.inv_keep(p)
        dxd = rnd(dx * m, dtype) if emulate else dx * m
    rows_in = torch.ones(rows, 1, dtype=dt)
    if fault == "trip_tail":
        nb = ln_blocks(rows, max_blocks)
        r0 = ((nb - 1) * 4 + 3) * 4
        rows_in[r0:r0 + 4] = 0
    tg, tb = d * xh * rows_in, d * rows_in
    dgamma, dbeta = tg.sum(0), tb.sum(0)
    if dgamma0 is not None:
        dgamma = dgamma0.to(dt) + dgamma
    if dbeta0 is not None:
        dbeta = dbeta0.to(dt) + dbeta
    out = dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dxd=dxd)
    if not emulate:   # sum |t| of the column sums, for summation_floor
        out["abs_dgamma"], out["abs_dbeta"] = tg.abs().sum(0), tb.abs().sum(0)
    return out


def ln_inputs(rows, cols, dtype, family, seed=0):
    """x, gamma, beta, dy (already rounded to dtype where the kernels read dtype).  family: 'randn' (x = randn * 2 + 0.5), 'hard'
    (a per-row offset large against the row's spread -- bf16: |offset| <= 8, spread >= 0.25; fp32: |offset| <= 100, spread >= 0.05 --
    and two or three channels scaled by 50), 'edge' (randn with row 0 the constant 1.5 and an all-zero dy row)."""
    g = torch.Generator().manual_seed(1000003 * rows + 101 * cols + seed)
    x = torch.randn(rows, cols, generator=g)
    if family == "hard":
        big, small = (8.0, 0.25) if dtype == torch.bfloat16 else (100.0, 0.05)
        off = (torch.rand(rows, 1, generator=g) * 2 - 1) * big
        spread = small + torch.rand(rows, 1, generator=g) * (2.0 - small)
        x = x * spread
        for c in torch.randperm(cols, generator=g)[:2 + cols % 2].tolist():
            x[:, c] *= 50.0
        x = x + off
    else:
        x = x * 2 + 0.5
    dy = torch.randn(rows, cols, generator=g)
    if family == "edge":
        x[0] = 1.5                       # every partial sum of the row is exact in fp32 (1.5 k, k <= 4096)
        dy[rows // 2] = 0.0
    gamma, beta = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    return x.to(dtype), gamma, beta, dy.to(dtype)


def ln_condition(x):
    """max over rows of |mean| / std (>= 1): how much a rounding of the mean is amplified in y."""
    xd = x.double()
    sd = xd.std(1, unbiased=False)
    ok = sd > 0
    return max(1.0, float((xd.mean(1).abs()[ok] / sd[ok]).max())) if ok.any() else 1.0


# A constant row c: fp64 gives y = beta exactly, xhat = 0.  In fp32 the mean is fl(fl(sum) * fl(1 / cols)) (or one division): with c = 1.5
# the sum is exact, which leaves two roundings, |mean - c| <= 2^-23 |c|, amplified by rstd = eps^-1/2:
#   |xhat| <= 2^-23 |c| eps^-1/2 =: delta;  y moves by <= delta |gamma|;  dx by <= rstd delta^2 max|g| per element through xhat * s2 (second
#   order: s2 itself is <= delta max|g|) and by as much again through rstd (var = mean((x - mean)^2) <= delta^2 eps, so rstd moves by
#   delta^2 / 2 of itself, times |g - s1| <= 2 max|g|);  dgamma[c] by <= delta |dy[row, c]|.
def constant_row_delta(c, eps):
    return 2.0 ** -23 * abs(c) / math.sqrt(eps)


# ---------------------------------------------------------------------------------------------------------------------------
# softmax with bucket bias, masks, dropout
# ---------------------------------------------------------------------------------------------------------------------------
def softmax_fwd_bwd(scores, qp, kpm, dP, dP_extra, BH, H, T, S, lds, maxrel, causal, p, seed, dtype=None, emulate=False, fault=None,
                    probs_bwd=None):
    """multihead_attention.py:343-386 as softmax.hip computes it.  scores [BH, T, lds], qp [BH, T, 2 maxrel] or None, kpm [B, S]
    (nonzero = padded) or None, dP [BH, T, lds] (gradient of the DROPPED probabilities), dP_extra fp32 [BH, T, S] or None (reaches the
    undropped probabilities).  Returns P, PD (P * mask / (1 - p); = P at p = 0), dS [BH, T, lds] with columns S.. exactly 0, and
    dQP [BH, T, 2 maxrel] (dS scattered by bucket) or None.  Rows without a visible key are zeros everywhere.
    probs_bwd: the probabilities the backward reads (default: this call's own, rounded in the emulation).
    fault: 'clip_low' | 'clip_high' (bucket clip off by one at one end), 'causal_no_offset', 'stride_S' (dropout counter stride)."""
    dt = torch.float32 if emulate else torch.float64
    B = BH // H
    i = torch.arange(T)[:, None]
    j = torch.arange(S)[None, :]
    lo, hi = -maxrel + (fault == "clip_low"), maxrel - 1 - (fault == "clip_high")
    bk = ((i - j).clamp(lo, hi) + maxrel) if qp is not None else None
    vis = torch.ones(T, S, dtype=torch.bool)
    if causal:
        vis = j <= i + (0 if fault == "causal_no_offset" else S - T)
    vis = vis[None].expand(BH, T, S)
    if kpm is not None:
        vis = vis & ~kpm.bool().repeat_interleave(H, 0)[:, None, :]
    x = scores[..., :S].to(dt)
    if qp is not None:
        x = x + torch.gather(qp.to(dt), 2, bk[None].expand(BH, T, S))
    x = x.masked_fill(~vis, -math.inf)
    m = x.max(2, keepdim=True).values
    live = torch.isfinite(m)
    m = torch.where(live, m, torch.zeros_like(m))
    if emulate:   # __expf(v) = v_exp_f32(v * log2 e); the denominator in lane order
        e = _t(np.exp2(((x - m).numpy() * LOG2E_F32).astype(np.float64)).astype(np.float32)).masked_fill(~vis, 0.0)
        l = _t(lane_order_sum(e.reshape(BH * T, S).numpy(), 8)).view(BH, T, 1)
    else:
        e = torch.exp(x - m).masked_fill(~vis, 0.0)
        l = e.sum(2, keepdim=True)
    inv = torch.where(l > 0, 1.0 / l.clamp_min(1e-300 if not emulate else 1e-38), torch.zeros_like(l))
    Pe = e * inv
    M = None
    if p > 0:
        M = _t(keep_mask_softmax(seed, p, BH * T, S, lds, S if fault == "stride_S" else None)).view(BH, T, S).to(dt) * A.inv_keep(p)
    PD = Pe * M if M is not None else Pe
    P = Pe
    if emulate:
        P, PD = rnd(Pe, dtype), rnd(PD, dtype)
    Pb = P if probs_bwd is None else probs_bwd[..., :S].to(dt)
    g = dP[..., :S].to(dt)
    if M is not None:
        g = g * M
    if dP_extra is not None:
        g = g + dP_extra.to(dt)
    t = g * Pb
    dot = _t(lane_order_sum(t.reshape(BH * T, S).numpy(), 8)).view(BH, T, 1) if emulate else t.sum(2, keepdim=True)
    dS = Pb * (g - dot)
    dQP = absQP = None
    if qp is not None:
        idx = bk[None].expand(BH, T, S)
        dQP = torch.zeros(BH, T, 2 * maxrel, dtype=dt).scatter_add_(2, idx, dS)
        if emulate:
            dQP = rnd(dQP, dtype)
        else:
            absQP = torch.zeros(BH, T, 2 * maxrel, dtype=dt).scatter_add_(2, idx, dS.abs())
    if emulate:
        dS = rnd(dS, dtype)

    def pad(a):
        return torch.cat([a, torch.zeros(BH, T, lds - S, dtype=a.dtype)], 2)
    return dict(P=pad(P), PD=pad(PD), dS=pad(dS), dQP=dQP, abs_dQP=absQP, live=live.view(BH, T))


def dropout_pattern_ok(PD, P, keep, p, S):
    """PD's zero pattern equals `keep` wherever P != 0, and the survivors are P / (1 - p) to two roundings of the type (the relative
    form of that needs a normal number: checked where P >= 2^-100)."""
    P, PD = P[..., :S].double(), PD[..., :S].double()
    keep = torch.as_tensor(np.asarray(keep)).reshape(P.shape)
    on = P != 0
    if not torch.equal((PD != 0)[on], keep[on]):
        return False
    want = P * A.inv_keep(p)
    return bool(torch.all(((PD - want).abs() <= 2.0 ** -7 * want)[(P >= 2.0 ** -100) & keep]))


def softmax_inputs(BH, H, T, S, lds, maxrel, dtype, scale=1.0, rel=True, lens=None, seed=0):
    g = torch.Generator().manual_seed(7919 * S + 31 * T + seed)
    scores = (torch.randn(BH, T, lds, generator=g) * scale).to(dtype)
    qp = (torch.randn(BH, T, 2 * maxrel, generator=g) * (0.5 * scale)).to(dtype) if rel else None
    dP = torch.randn(BH, T, lds, generator=g).to(dtype)
    extra = torch.randn(BH, T, S, generator=g) * 0.1
    kpm = None
    if lens is not None:
        kpm = torch.zeros(BH // H, S, dtype=torch.uint8)
        for b, n in enumerate(lens):
            kpm[b, n:] = 1
    return scores, qp, kpm, dP, extra


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm1d + activation + dropout (+ residual) over channels-last rows
# ---------------------------------------------------------------------------------------------------------------------------
def bn_geometry(rows, C):
    """batchnorm.hip: rows per block iteration, blocks of the partial-sum kernels (cap 64)."""
    rg = 256 // (C // 4)
    return rg, min(max((rows + rg * 16 - 1) // (rg * 16), 1), 64)


def _fma(a, b, c, emulate):
    """a * b + c; in the emulation rounded once, as the v_fma_f32 hipcc contracts xhat * gamma + beta and 1 - y * y of batchnorm.hip into
    (profiles/norm_fp64_isa_excerpts.txt).  1 - tanh^2 cancels, so whether y * y is rounded first decides the last bits of the factor."""
    return (a.double() * b.double() + c.double()).float() if emulate else a * b + c


def batchnorm_fwd(x, gamma, beta, running_mean, running_var, nbt, momentum, eps, training, tanh, p, seed, residual=None, y_f32=True,
                  dtype=torch.float32, emulate=False, fault=None):
    """x fp32 [rows, C].  Returns y [rows, C] (dropout(act(BN(x))) + residual; rounded to dtype in the emulation unless y_f32), mean,
    rstd, and the running mean / var / batch counter after the call (training: momentum blend with the UNBIASED batch variance,
    counter + 1; eval: untouched, statistics taken from them).  fault: 'skip_block' (the last partial-sum block never reaches the
    statistics)."""
    rows, C = x.shape
    dt = torch.float32 if emulate else torch.float64
    xd = x.double()
    eps = float(F32(eps))
    rm = rv = None
    if training:
        use = torch.ones(rows, 1, dtype=torch.float64)
        if fault == "skip_block":
            rg, nblk = bn_geometry(rows, C)
            r = torch.arange(rows)
            use[(r // rg) % nblk == nblk - 1] = 0
        mean = (xd * use).sum(0) / rows
        var = ((xd * xd * use).sum(0) / rows - mean * mean).clamp_min(0)           # the kernel's fp64 stage: E[x^2] - mean^2
        if not emulate:
            var = ((xd - mean) ** 2).mean(0)
        rstd = 1.0 / torch.sqrt(var + eps)
        if running_mean is not None:
            unb = var * rows / (rows - 1) if rows > 1 else var
            mom = float(F32(momentum))
            if emulate:
                rm = (1 - F32(momentum)).item() * running_mean.float() + mom * mean.float()
                rv = (1 - F32(momentum)).item() * running_var.float() + mom * unb.float()
            else:
                rm = (1 - mom) * running_mean.double() + mom * mean
                rv = (1 - mom) * running_var.double() + mom * unb
        nbt = nbt + 1
    else:
        mean = running_mean.double()
        rstd = 1.0 / torch.sqrt((running_var.float() + F32(eps).item()).double()) if emulate else 1.0 / torch.sqrt(running_var.double() + eps)
        rm, rv = running_mean.to(dt), running_var.to(dt)
    mean, rstd = mean.to(dt), rstd.to(dt)
    y = _fma((x.to(dt) - mean) * rstd, gamma.to(dt), beta.to(dt), emulate)
    if tanh:
        y = torch.tanh(y)
    if p > 0:
        y = y * (_t(keep_mask_rows(seed, p, rows, C)).to(dt) * A.inv_keep(p))
    if residual is not None:
        y = y + residual.to(dt)
    if emulate and not y_f32:
        y = rnd(y, dtype)
    return dict(y=y, mean=mean, rstd=rstd, running_mean=rm, running_var=rv, nbt=nbt)


def batchnorm_bwd(x, dy, mean, rstd, gamma, beta, training, tanh, p, seed, dtype=torch.float32, emulate=False, dgamma0=None, dbeta0=None):
    """dx [rows, C], dgamma, dbeta (accumulated) of batchnorm_fwd without the residual.  g = mask * dy * act'(z);
    training: dx = gamma rstd (g - mean(g) - xhat mean(g xhat)); eval: dx = gamma rstd g.  dbeta += sum g, dgamma += sum g xhat
    (fp64 sums of the fp32 terms, then one cast, in the emulation)."""
    rows, C = x.shape
    dt = torch.float32 if emulate else torch.float64
    ga, be = gamma.to(dt), beta.to(dt)
    xh = (x.to(dt) - mean.to(dt)) * rstd.to(dt)
    g = dy.to(dt)
    if p > 0:
        g = g * (_t(keep_mask_rows(seed, p, rows, C)).to(dt) * A.inv_keep(p))
    abs1, abs2 = g.double().abs().sum(0), (g.double() * xh.double()).abs().sum(0)     # sum |t| with act' <= 1, for summation_floor
    if tanh:
        yv = torch.tanh(_fma(xh, ga, be, emulate))
        g = g * _fma(-yv, yv, torch.ones_like(yv), emulate)
    s1, s2 = g.double().sum(0), (g.double() * xh.double()).sum(0)
    m1, m2 = (s1 / rows).to(dt), (s2 / rows).to(dt)
    if not training:
        m1, m2 = torch.zeros_like(m1), torch.zeros_like(m2)
    dx = ga * rstd.to(dt) * (g - m1 - xh * m2)
    if emulate:
        dx = rnd(dx, dtype)
    dgamma, dbeta = s2.to(dt), s1.to(dt)
    if dgamma0 is not None:
        dgamma = dgamma0.to(dt) + dgamma
    if dbeta0 is not None:
        dbeta = dbeta0.to(dt) + dbeta
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, abs_dgamma=abs2, abs_dbeta=abs1)


def place_rows(y, L, pad, bstride, fill, dtype, fault=None):
    """The mapped layout of batchnorm.hip: row r of y [rows, C] goes to element (r // L) * bstride + (pad + r % L) * C of a flat buffer,
    `pad` zeroed halo rows in front of and behind every batch block, everything else (the gap up to bstride) keeps `fill`.
    fault: 'halo_short' (the last halo row behind a block is not written)."""
    rows, C = y.shape
    nb = rows // L
    out = torch.full((nb, bstride), fill, dtype=dtype)
    body = out[:, :(L + 2 * pad) * C].view(nb, L + 2 * pad, C)
    body[:] = 0
    body[:, pad:pad + L] = y.view(nb, L, C).to(dtype)
    if fault == "halo_short":
        body[:, -1] = fill
    return out.view(-1)


def mapped_layout_ok(buf, nbatch, C, L, pad, bstride, fill):
    """Halo rows exactly zero and every element between the batch blocks still `fill`, bit for bit."""
    b = buf.view(nbatch, bstride)
    body = b[:, :(L + 2 * pad) * C].reshape(nbatch, L + 2 * pad, C)
    halo = torch.cat([body[:, :pad], body[:, pad + L:]], 1).float()
    gap = b[:, (L + 2 * pad) * C:].float()
    return bool(torch.all(halo == 0) and torch.all(gap == fill))


def extract_rows(buf, nbatch, C, L, pad, bstride):
    return buf.view(nbatch, bstride)[:, :(L + 2 * pad) * C].reshape(nbatch, L + 2 * pad, C)[:, pad:pad + L].reshape(nbatch * L, C)


def bn_inputs(rows, C, seed=0, far=True):
    """x fp32 [rows, C] (every fourth channel with mean 50 and spread 0.1 when `far`), dy, gamma, beta, residual, running mean / var."""
    g = torch.Generator().manual_seed(65537 * C + rows + seed)
    x = torch.randn(rows, C, generator=g) * 1.5 + torch.randn(C, generator=g)
    if far:
        x[:, 1::4] = 50.0 + 0.1 * torch.randn(rows, len(range(1, C, 4)), generator=g)
    dy = torch.randn(rows, C, generator=g)
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.3
    res = torch.randn(rows, C, generator=g)
    rmean = x.mean(0) + 0.1 * torch.randn(C, generator=g)
    rvar = x.var(0, unbiased=False).clamp_min(1e-3) * (1 + 0.1 * torch.rand(C, generator=g))
    return x, dy, gamma, beta, res, rmean, rvar


# ---------------------------------------------------------------------------------------------------------------------------
# metric and bars
# ---------------------------------------------------------------------------------------------------------------------------
def _rows(t):
    t = t.double()
    return t.reshape(-1, 1) if t.dim() == 1 else t.reshape(-1, t.shape[-1])


def row_errors(got, ref, slack=None):
    """Per row: ||got - ref|| / max(||ref row||, 2^-8 * largest row norm) (a 1-D tensor counts as rows of one element: the per-column
    form of the reduced quantities), after `slack` -- a derived absolute bound on the row's error norm that no rounding model covers
    (constant rows) -- is taken off.  A row with zero error counts 0 whatever its norm."""
    got, ref = _rows(got), _rows(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rn = ref.norm(dim=1)
    den = torch.clamp(rn, min=2.0 ** -8 * rn.max().item())
    err = (got - ref).norm(dim=1)
    if slack is not None:
        err = (err - slack.double().reshape(-1)).clamp_min(0)
    return torch.where(err == 0, torch.zeros_like(err), err / den.clamp(min=1e-300)), den


def row_metric(got, ref, slack=None):
    return row_errors(got, ref, slack)[0].max().item()


def summation_floor(abs_sum, chain, extra=None):
    """gamma_n * sum |t| (+ extra): the deterministic bound on an fp32 sum of the terms t in ANY order whose longest addition chain
    has n links, gamma_n = n u / (1 - n u), u = 2^-24, one more link for the rounding of each term itself.  abs_sum comes from the fp64
    reference, never from the kernel."""
    n = chain + 1
    f = n * U32 / (1 - n * U32) * abs_sum.double()
    return f if extra is None else f + extra.double()


def passes(got, ref, emu, slack=None, floor=None, select=None):
    """(ok, kernel worst row, emulation worst row).  ok: every row of `got` is within BAR x the emulation's worst row of `ref` --
    or, for the sums over rows, within `floor` (summation_floor, absolute, per element) where that is larger.  select: bool mask of the
    rows that take part (the others are checked by the caller).  Non-finite values fail."""
    if not torch.isfinite(got.double()).all():
        return False, math.inf, row_metric(emu, ref, slack)
    ek, den = row_errors(got, ref, slack)
    ee, _ = row_errors(emu, ref, slack)
    if select is not None:
        ek, ee, den = ek[select.reshape(-1)], ee[select.reshape(-1)], den[select.reshape(-1)]
    e_e = ee.max().item()
    lim = torch.full_like(ek, BAR * e_e)
    if floor is not None:
        fl = floor.double().reshape(-1)
        if select is not None:
            fl = fl[select.reshape(-1)]
        lim = torch.maximum(lim, fl / den.clamp(min=1e-300))
    return bool((ek <= lim).all()), ek.max().item(), e_e
