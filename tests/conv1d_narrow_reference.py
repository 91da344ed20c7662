"""Plain reference of the narrow Conv1d family (csrc/conv1d_narrow.hip: st5_conv1d_narrow, st5_conv1d_cout1), the yardstick
tests/test_conv1d_narrow_fp64_gpu.py holds every kernel of the family to.  One function, `conv`, takes what the C ABI takes -- FLAT
buffers plus the ABI's strides, not pre-sliced tensors -- and comes in two forms:

- fp64 (emulate=False): the truth.  The header's formula on the bf16-rounded inputs, in double, addresses as plain index arithmetic,
      y[b, t, co] = act(alpha * sum_{tau, c} w[co, tau Cin + c] x[x_off + b x_bs + t x_ts + tau tap_stride + c] + bias[co])
                    + R[r_off + b r_bs + t r_ts + co] + beta * y_old[y_off + b y_bs + t y_ts + co]
  with the LeakyReLU slopes the fp32 constants the kernels hold (gemm_reference._SLOPE); st5_conv1d_cout1 is the same with one output
  channel, y dense ([B * L]), no residual / beta, and its activation through gemm_reference.act64.
- emulation (emulate=True): the same arithmetic with the kernels' rounding points -- fp32 accumulation, every epilogue step its own fp32
  operation in each form's order (direct form conv1d_narrow_kernel: acc * alpha, then + bias; staged form conv1d_narrow32_kernel and
  cout1: ONE fmaf(acc, alpha, bias)), then the slope, + R, + beta * y_old (a product, then a sum), one bf16 rounding of the result.
  `fault=` plants one wrong-kernel behaviour (FAULTS; accepted by the fp64 form too, for `decides`);
  tests/test_conv1d_narrow_reference_cpu.py shows that every one of them fails the bar.

The bar is gemm_reference's (bar_terms / bar_ratio), per element, nothing in it from a kernel:
      |got - ref64| <= BAR max(|emu - ref64|, ulp_bf16(ref64) / 2) + summation_floor(S, chain)
BAR = norm_reference.BAR, S = |alpha| sum |w| |x| + |bias| + |R| + |beta y_old| (every activation here has slope <= 1), chain = taps * Cin +
gemm_reference.EPILOGUE_OPS.  `conv_transpose64` restates ConvTranspose1d (k = 2 s, padding = s / 2) in double for the phase tests.
Everything is torch index arithmetic, so the same functions run on the GPU for the cases that are judged there (batch chunks b0:b1)."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests import gemm_reference as G
from tests import norm_reference as NR

BAR = NR.BAR
F32 = np.float32
BF = torch.bfloat16
ACT_NONE, ACT_TANH, ACT_LRELU_01, ACT_LRELU_001 = G.ACT_NONE, G.ACT_TANH, G.ACT_LRELU_01, G.ACT_LRELU_001
GUARD, NAN = G.GUARD, G.NAN
TILE_T = {1: 1024, 2: 512}          # time steps per block tile by CB = Cout / 32
WAVE_T = {1: 128, 2: 64}            # ... per wave
LDS_LIMIT = 160 * 1024

FAULTS = ("tap_late", "last_tap_dropped", "dilation_1", "bias_before_alpha", "slope_01", "r_row", "beta_ignored", "half_swap", "tblock_swap",
          "half16_swap", "y_bs_dense", "phase_t_off")
EPILOGUE_FAULTS = ("bias_before_alpha", "slope_01", "r_row", "beta_ignored")


def problem(x, w, y, B, L, Cin, Cout, taps, tap_stride, x_bs, x_ts, y_bs, y_ts, **kw):
    """Arguments of st5_conv1d_narrow (Cout = 1: st5_conv1d_cout1 with y_bs = L, y_ts = 1).  x, y, R: flat bf16 tensors with *_off the
    element offset of the pointer handed to the library; w: flat bf16 [Cout * taps * Cin]; bias: fp32 [Cout] or None."""
    p = SimpleNamespace(x=x, w=w, y=y, B=B, L=L, Cin=Cin, Cout=Cout, taps=taps, tap_stride=tap_stride, x_bs=x_bs, x_ts=x_ts, y_bs=y_bs,
                        y_ts=y_ts, x_off=0, y_off=0, bias=None, R=None, r_off=0, r_bs=0, r_ts=0, alpha=1.0, beta=0.0, act=ACT_NONE)
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


# ---------------------------------------------------------------------------------------------------------------------------
# the dispatch, restated (csrc/conv1d_narrow.hip narrow_plan; buffers 16-byte aligned at element 0)
# ---------------------------------------------------------------------------------------------------------------------------
def staged_lds(Cin, taps, tap_rows):
    """Bytes of the staged form's LDS image: weights [32][taps Cin + 8] bf16, then 8 waves x (128 + (taps - 1) tap_rows) rows of
    2 Cin + 16 bytes."""
    up16 = lambda n: (n + 15) // 16 * 16
    return up16(32 * (taps * Cin + 8) * 2) + 8 * up16((128 + (taps - 1) * tap_rows) * (2 * Cin + 16))


def tiles_per_block(B, L, CB):
    tiles = (L + TILE_T[CB] - 1) // TILE_T[CB]
    n = 1
    while n < 8 and B * (tiles // (n * 2)) >= 1024:
        n *= 2
    return n


def plan(p):
    """[staged, CB, NJ, tiles_per_block, time steps per block tile, LDS bytes] as st5_conv1d_narrow_plan reports them."""
    CB, NJ, K = p.Cout // 32, p.Cin // 16, p.taps * p.Cin
    vec16 = p.y_off % 8 == 0 and p.y_ts % 8 == 0 and p.y_bs % 8 == 0 and (p.R is None or (p.r_off % 8 == 0 and p.r_ts % 8 == 0 and p.r_bs % 8 == 0))
    staged, lds = 0, CB * 32 * (K + 8) * 2
    if p.Cout == 32 and vec16 and p.x_ts == p.Cin and p.tap_stride % p.Cin == 0 and p.Cin in (32, 64):
        s = staged_lds(p.Cin, p.taps, p.tap_stride // p.Cin)
        if s <= LDS_LIMIT:
            staged, lds = 1, s
    return [staged, CB, NJ, tiles_per_block(p.B, p.L, CB), TILE_T[CB], lds]


def form_of(p):
    return "cout1" if p.Cout == 1 else "staged" if plan(p)[0] else "direct"


# ---------------------------------------------------------------------------------------------------------------------------
# addressing
# ---------------------------------------------------------------------------------------------------------------------------
def _ar(n, dev):
    return torch.arange(n, dtype=torch.int64, device=dev)


def x_offsets(p, b0, b1, dev, fault=None):
    """[nb, L, taps, Cin] element offsets x_off + b x_bs + t x_ts + tau tap_stride + c."""
    tap_stride = p.x_ts if fault == "dilation_1" else p.tap_stride
    x_off = p.x_ts - p.x_off if fault == "phase_t_off" else p.x_off
    tau = _ar(p.taps, dev) * tap_stride
    if fault == "tap_late":
        tau[0] += p.x_ts
    return x_off + ((b0 + _ar(b1 - b0, dev)) * p.x_bs)[:, None, None, None] + (_ar(p.L, dev) * p.x_ts)[None, :, None, None] \
        + tau[None, None, :, None] + _ar(p.Cin, dev)[None, None, None, :]


def c_offsets(off, bs, ts, b0, b1, L, Cout, dev, row_shift=0):
    """[nb, L, Cout] element offsets off + b bs + t ts + co (row_shift: row (t + shift) mod L instead)."""
    t = (_ar(L, dev) + row_shift) % L
    return off + ((b0 + _ar(b1 - b0, dev)) * bs)[:, None, None] + (t * ts)[None, :, None] + _ar(Cout, dev)[None, None, :]


def y_offsets(p, b0=0, b1=None, dev="cpu"):
    return c_offsets(p.y_off, p.y_bs, p.y_ts, b0, p.B if b1 is None else b1, p.L, p.Cout, dev)


# ---------------------------------------------------------------------------------------------------------------------------
# the operation
# ---------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _swap(y, dim, n, lo, hi):
    """Blocks [lo, lo + n) and [hi, hi + n) of dimension `dim` exchanged (where both exist)."""
    if y.shape[dim] < hi + n:
        return y
    idx = torch.arange(y.shape[dim], device=y.device)
    idx[lo:lo + n], idx[hi:hi + n] = torch.arange(hi, hi + n, device=y.device), torch.arange(lo, lo + n, device=y.device)
    return y.index_select(dim, idx)


def conv(p, emulate=False, form=None, fault=None, b0=0, b1=None):
    """Batches [b0, b1) of the result as a double tensor y [nb, L, Cout] -- the value each output element holds after the call (the
    emulation's rounded to bf16).  From the fp64 form also S (sum of absolute terms behind every element), chain and pre (the value in
    front of the activation)."""
    assert fault is None or fault in FAULTS, fault
    form = form or form_of(p)
    b1 = p.B if b1 is None else b1
    dev = p.x.device
    dt = torch.float32 if emulate else torch.float64
    K = p.taps * p.Cin
    alpha, beta = float(F32(p.alpha)), float(F32(p.beta))
    X = p.x[x_offsets(p, b0, b1, dev, fault)].reshape(b1 - b0, p.L, K)
    W = p.w.reshape(p.Cout, K)
    Xd, Wd = X.double(), W.double()
    if fault == "last_tap_dropped":
        Xd = Xd.clone()
        Xd[:, :, K - p.Cin:] = 0
    if emulate:       # fp32 accumulation (on the GPU: the exact sum rounded once, so that no project kernel and no BLAS mode is involved)
        acc = (Xd @ Wd.t()).float() if dev.type != "cpu" else Xd.float() @ Wd.float().t()
    else:
        acc = Xd @ Wd.t()
    bias = p.bias.to(dt)[None, None, :] if p.bias is not None else None
    if fault == "bias_before_alpha" and bias is not None:
        pre = (acc + bias) * alpha
    elif emulate and form in ("staged", "cout1"):
        pre = _fma32(acc, torch.tensor(alpha, dtype=dt, device=dev), bias if bias is not None else torch.zeros((), dtype=dt, device=dev))
    else:
        pre = acc * alpha
        if bias is not None:
            pre = pre + bias
    if form == "cout1":
        v = G.act64(p.act, pre)
    else:
        act = ACT_LRELU_01 if fault == "slope_01" and p.act == ACT_LRELU_001 else p.act
        assert act in (ACT_NONE, ACT_LRELU_01, ACT_LRELU_001)
        v = torch.where(pre > 0, pre, pre * G._SLOPE[act]) if act in G._SLOPE else pre
    Rm = old = None
    if p.R is not None:
        Rm = p.R[c_offsets(p.r_off, p.r_bs, p.r_ts, b0, b1, p.L, p.Cout, dev, 1 if fault == "r_row" else 0)].to(dt)
        v = v + Rm
    if beta != 0:
        old = p.y[y_offsets(p, b0, b1, dev)].to(dt)
        if fault != "beta_ignored":
            v = v + beta * old
    y = NR.rnd(v, BF).double() if emulate else v
    if fault == "half_swap":            # the two 4-channel halves of every 8-channel group
        y = y[:, :, torch.arange(p.Cout, device=dev) ^ 4]
    elif fault == "tblock_swap":        # the first two 32-step time blocks
        y = _swap(y, 1, 32, 0, 32)
    elif fault == "half16_swap":        # the two 16-row halves of the first 32-step block
        y = _swap(y, 1, 16, 0, 16)
    elif fault == "y_bs_dense":         # written with batch stride L * Cout: what then stands at the right addresses
        img = p.y.double().clone()
        img[c_offsets(p.y_off, p.L * p.Cout, p.y_ts, b0, b1, p.L, p.Cout, dev)] = y
        y = img[y_offsets(p, b0, b1, dev)]
    out = SimpleNamespace(y=y, form=form)
    if not emulate:
        S = abs(alpha) * (Xd.abs() @ Wd.abs().t())
        if bias is not None:
            S = S + bias.abs()
        if Rm is not None:
            S = S + Rm.abs()
        if old is not None:
            S = S + (beta * old).abs()
        out.S, out.chain, out.pre = S, K + G.EPILOGUE_OPS, pre
    return out


def conv_transpose64(x, w, bias, s):
    """ConvTranspose1d with kernel 2 s, stride s, padding s / 2, in double: x [B, L, Cin], w [Cin, Cout, 2 s], bias [Cout] ->
    [B, s L, Cout];  out[b, s t + j - s / 2, co] += sum_ci x[b, t, ci] w[ci, co, j]  wherever that row exists."""
    B, L, _ = x.shape
    out = bias.double()[None, None, :].repeat(B, s * L, 1)
    xd, wd = x.double(), w.double()
    t = torch.arange(L)
    for j in range(2 * s):
        row = s * t + j - s // 2
        ok = (row >= 0) & (row < s * L)
        out[:, row[ok]] += xd[:, t[ok]] @ wd[:, :, j]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the bar
# ---------------------------------------------------------------------------------------------------------------------------
def expect(p, form=None, b0=0, b1=None):
    """ref (fp64), emulation, (den, floor) of the bar and the tolerance, per output element of batches [b0, b1)."""
    ref, emu = conv(p, form=form, b0=b0, b1=b1), conv(p, emulate=True, form=form, b0=b0, b1=b1)
    den, floor = G.bar_terms(ref.y, emu.y, ref.S, ref.chain, BF)
    return SimpleNamespace(ref=ref.y, emu=emu.y, den=den, floor=floor, tol=BAR * den + floor, pre=ref.pre, form=emu.form,
                           emu_err=(emu.y - ref.y).abs().max().item())


def ratio(got, e):
    """Worst (|got - ref| - floor) / den over the elements: passes <=> <= BAR (non-finite: inf)."""
    return G.bar_ratio(got.double(), e.ref, e.den, e.floor).max().item()


def decides(p, e, fault, form=None):
    """Share of the elements the epilogue fault concerns (slope_01: those with a negative value in front of the activation; the
    others: all) on which it would move the result by less than 8 x the element's tolerance -- gemm_reference.mask_decides'
    condition, from the reference alone.  (share, number of elements concerned)"""
    delta = (conv(p, form=form, fault=fault).y - e.ref).abs()
    sel = e.pre < 0 if fault == "slope_01" else torch.ones_like(delta, dtype=torch.bool)
    return (delta[sel] < 8 * e.tol[sel]).double().mean().item(), int(sel.sum())


def bits(t):
    return t.view(torch.int16)


def untouched(p, before, after):
    """Number of elements outside the output (columns between Cout and y_ts, halo rows, other phases, gaps between batches, the guard)
    whose bits changed."""
    free = torch.ones(before.numel(), dtype=torch.bool, device=before.device)
    free[y_offsets(p, dev=before.device).reshape(-1)] = False
    return int(((bits(before) != bits(after)) & free).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# case generators shared by tests/test_conv1d_narrow_reference_cpu.py and tests/test_conv1d_narrow_fp64_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------
# LeakyReLU(0.01) cases keep taps * Cin <= 96: a negative output is 0.01 pre, while the summation floor grows like K^1.5 u (K terms of
# either sign: sum |w| |x| ~ sqrt K x the spread of the sum).  From K = 128 on the floor alone hides the slope on more than 1 % of the negative
# elements (tests/test_conv1d_narrow_reference_cpu.py asserts the share at the combinations in use).
LRELU001_MAX_K = 96
KINDS = ("plain", "bias_alpha_lrelu01", "lrelu001", "res", "beta1", "beta05", "res_beta", "res_strided", "halo", "phase")
Y_LAYOUTS = ("plain", "pad4", "pad8", "halo", "phase")


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1000003, 7919, 104729, 31, 611953, 17, 257, 65537, 3))) + 12345)


def _signed(g, shape, lo, hi, alternate_rows=False):
    """Magnitudes uniform in [lo, hi) (exact in bf16 after rounding, both signs): random signs, or the sign alternating from row to row
    (dimension 1) so that a value taken from the neighbouring row differs by at least 2 lo."""
    mag = lo + (hi - lo) * torch.rand(shape, generator=g)
    if alternate_rows:
        sign = (1 - 2 * (torch.arange(shape[1]) % 2)).double().view(1, -1, 1).float() * (1 - 2 * torch.randint(0, 2, (shape[0], 1, shape[2]), generator=g)).float()
    else:
        sign = (1 - 2 * torch.randint(0, 2, shape, generator=g)).float()
    return mag * sign


def _scatter(n, offs, values, fill=NAN):
    buf = torch.full((n,), fill, dtype=BF)
    if values is not None:
        buf[offs.reshape(-1)] = values.reshape(-1).to(BF)
    return buf


def case(Cin, Cout, taps, dil, L, B, kind="plain", x_pad=0, x_gap=None, y_layout=None, r_pad=None, phase=(4, 1), halo=3, seed=0):
    """One problem.  x: [B][L + (taps - 1) dil rows][Cin + x_pad] with NaN in the row padding, in the x_gap elements between
    batches (default 16 when B > 1) and in GUARD elements behind the last row; values N(0, 1), weights N(0, 1) 2 / sqrt(taps Cin) (the
    sum has spread 2), bias 1 + 0.1 N(0, 1).  kind (KINDS) chooses the epilogue: alpha 0.5 where there is a bias, residual magnitudes in
    [1, 1.5) with the sign alternating by row, old output contents of magnitude [2, 3).  y_layout (Y_LAYOUTS): plain; pad4 / pad8 (row
    padding of 4 / 8 elements and as much between batches); halo (`halo` rows in front of and behind each batch); phase = (s, r): every
    s-th row from row offset r.  Everything outside the output elements is NaN, GUARD elements behind."""
    assert kind in KINDS, kind
    assert kind != "lrelu001" or taps * Cin <= LRELU001_MAX_K, "see LRELU001_MAX_K"
    g = _gen(Cin, Cout, taps, dil, L, B, KINDS.index(kind), x_pad, seed)
    K = taps * Cin
    rows = L + (taps - 1) * dil
    x_ts = Cin + x_pad
    x_gap = (16 if B > 1 else 0) if x_gap is None else x_gap
    x_bs = rows * x_ts + x_gap
    xo = c_offsets(0, x_bs, x_ts, 0, B, rows, Cin, "cpu")
    x = _scatter(int(xo.max()) + 1 + GUARD, xo, torch.randn(B, rows, Cin, generator=g))
    w = (torch.randn(Cout, K, generator=g) * (2.0 / math.sqrt(K))).to(BF).reshape(-1)
    bias = 1.0 + 0.1 * torch.randn(Cout, generator=g)
    y_layout = y_layout or {"halo": "halo", "phase": "phase"}.get(kind, "plain")
    assert y_layout in Y_LAYOUTS
    if y_layout == "plain":
        y_off, y_ts, y_bs = 0, Cout, L * Cout
    elif y_layout in ("pad4", "pad8"):
        q = 4 if y_layout == "pad4" else 8
        y_off, y_ts, y_bs = 0, Cout + q, L * (Cout + q) + q
    elif y_layout == "halo":
        y_off, y_ts, y_bs = halo * Cout, Cout, (L + 2 * halo) * Cout
    else:
        s, r = phase
        y_off, y_ts, y_bs = r * Cout, s * Cout, L * s * Cout
    kw = dict(y_off=y_off)
    if kind in ("bias_alpha_lrelu01", "lrelu001"):
        kw.update(bias=bias, alpha=0.5, act=ACT_LRELU_01 if kind == "bias_alpha_lrelu01" else ACT_LRELU_001)
    elif kind != "plain":
        kw.update(bias=bias, alpha=0.5)
    yo = c_offsets(y_off, y_bs, y_ts, 0, B, L, Cout, "cpu")
    ny = max(int(yo.max()) + 1, B * y_bs) + GUARD
    old = None
    if kind in ("beta1", "beta05", "res_beta"):
        kw.update(beta=0.5 if kind == "beta05" else 1.0)
        old = _signed(g, (B, L, Cout), 2.0, 3.0)
    y = _scatter(ny, yo, old)
    if kind in ("res", "res_beta", "res_strided"):
        r_pad = (8 if kind == "res_strided" else 0) if r_pad is None else r_pad
        r_ts, r_bs = Cout + r_pad, L * (Cout + r_pad) + r_pad
        ro = c_offsets(0, r_bs, r_ts, 0, B, L, Cout, "cpu")
        kw.update(R=_scatter(int(ro.max()) + 1 + GUARD, ro, _signed(g, (B, L, Cout), 1.0, 1.5, alternate_rows=True)), r_bs=r_bs, r_ts=r_ts)
    return problem(x, w, y, B, L, Cin, Cout, taps, dil * x_ts, x_bs, x_ts, y_bs, y_ts, **kw)


def cout1_case(Cin, taps, L, B, act=ACT_TANH, x_pad=0, seed=0):
    """st5_conv1d_cout1: alpha 0.25, bias about 1, x as in `case`; y dense [B * L], NaN with GUARD elements behind."""
    g = _gen(Cin, 1, taps, 1, L, B, act, x_pad, seed)
    K = taps * Cin
    rows, x_ts = L + taps - 1, Cin + x_pad
    x_bs = rows * x_ts + (16 if B > 1 else 0)
    xo = c_offsets(0, x_bs, x_ts, 0, B, rows, Cin, "cpu")
    x = _scatter(int(xo.max()) + 1 + GUARD, xo, torch.randn(B, rows, Cin, generator=g))
    w = (torch.randn(K, generator=g) * (4.0 / math.sqrt(K))).to(BF)
    y = torch.full((B * L + GUARD,), NAN, dtype=BF)
    return problem(x, w, y, B, L, Cin, 1, taps, x_ts, x_bs, x_ts, L, 1, bias=1.0 + 0.1 * torch.randn(1, generator=g), alpha=0.25, act=act)


def transpose_inputs(Cin, Cout, s, L, B, seed=0):
    """x [B, L, Cin] and the ConvTranspose1d parameters w [Cin, Cout, 2 s], bias [Cout], all bf16-exact fp32."""
    g = _gen(Cin, Cout, s, L, B, seed)
    r = lambda t: t.to(BF).float()
    return r(torch.randn(B, L, Cin, generator=g)), r(torch.randn(Cin, Cout, 2 * s, generator=g) * (2.0 / math.sqrt(2 * Cin))), \
        r(1.0 + 0.1 * torch.randn(Cout, generator=g))


def transpose_phases(x, w, bias, s):
    """The s phase problems of conv_transpose64 on ONE output buffer, as speecht5_amd.hifigan.conv_transpose1d poses them: phase r is a
    2-tap convolution over rows [t + t_off, t + t_off + 1] of the input padded by one zero row on each side, weights
    [w[:, :, j1 + s]; w[:, :, j1]] with j1 = (r + s / 2) mod s, written to rows s t + r.  The y buffer holds NaN."""
    B, L, Cin = x.shape
    Cout = w.shape[1]
    xp = torch.zeros(B, L + 2, Cin)
    xp[:, 1:L + 1] = x
    xf = torch.cat([xp.reshape(-1), torch.full((GUARD,), NAN)]).to(BF)
    y = torch.full((B * L * s * Cout + GUARD,), NAN, dtype=BF)
    out = []
    for r in range(s):
        j1 = (r + s // 2) % s
        t_off = 0 if r < s - s // 2 else 1
        wr = torch.cat([w[:, :, j1 + s], w[:, :, j1]], 0).t().contiguous().to(BF).reshape(-1)
        out.append(problem(xf, wr, y, B, L, Cin, Cout, 2, Cin, (L + 2) * Cin, Cin, L * s * Cout, s * Cout, x_off=t_off * Cin, y_off=r * Cout,
                           bias=bias.float()))
    return out
