"""Plain reference of csrc/conv0.hip -- Conv1d(1 -> C, k, stride, no bias) + GroupNorm(C groups: statistics per (clip, channel) over
time) + GELU, channels-last -- the yardstick tests/test_conv0_fp64_gpu.py holds st5_conv0_gn_gelu_fwd / _bwd to.  Written from the
header comment of conv0.hip (lines 1-18) and the entry points in include/speecht5_hip.h, not from the kernels.  Conventions (U32,
gamma(k), summation_floor, BAR, rnd) are tests/norm_reference.py's and tests/elementwise_reference.py's.

a. fp64 truth (forward_truth, backward_truth): explicit formulas in torch double on the already-rounded fp32 / bf16 inputs, no autograd
   (tests/test_conv0_reference_cpu.py pins them to F.conv1d + F.group_norm + F.gelu and its autograd).

b. Cancellation magnitudes, all from the truth.  The layer never forms the convolution to take its statistics: with the waveform moments
   M_j = sum_t x[s t + j], R_jj' = sum_t x[s t + j] x[s t + j'] it uses mean = w.M / L, var = w^T R w / L - mean^2, and the backward folds
   GroupNorm in afterwards, dw_j = rstd gamma [A_j - S1 M_j / L - S2 rstd (R w - mean M)_j / L].  Each is a difference of large terms on a
   correlated waveform.  What an fp32 rounding is relative to:
     T1[b,c] = sum_j |w_j| sum_t |x_j| / L,   T2[b,c] = sum_jj' |w_j||w_j'| sum_t |x_j x_j'| / L,   kappa = T2 / var;
     Mag[c,j] = sum_b rstd |gamma| (sum_t |dz x_j| + |S1 M_j| / L + |S2| rstd |(R w - mean M)_j| / L);   sum_t |dz x_hat|, sum_t |dz|.

c. Allowances -- every one derived, none read from a kernel's output (u = 2^-24, gamma_n = n u / (1 - n u)).
   Moments.  A chunk partial is an fp32 sum of at most 1024 fused products whose longest chain has 12 links (4 frames of a thread, 6 wave
     steps, 2 block adds); the fold over chunks is fp64.  Class D with chain 12: |dM_j| <= summation_floor(sum_t |x_j|, 12), likewise R.
   Statistics.  dmean = summation_floor(T1, 12) + u |mean| (the moments, and the cast of the saved mean);
     dvar = summation_floor(T2 + 2 |mean| T1, 12) (w^T R w / L, and mean^2 through 2 |mean| dmean);
     the saved rstd lies in [rstd(var + dvar), rstd(max(var - dvar, 0))], widened by one fp32 ulp (its cast).
   Forward, per element: the sum of
     1. the statistics allowance through the affine and GELU: |gamma| (|x_hat| drstd / rstd + rstd dmean) sup|gelu'|  (sup gelu' = 1.129);
     2. the apply pass on the true statistics.  a = sum_j |sc w_j x_j| + |sh| (sc = rstd gamma, sh = beta - mean sc) is what the
        pre-activation z is rounded against;
        fp32 / VALU: BAR x the error of a plain fp32 emulation of the documented apply (k fused multiply-adds, one for the affine, erf):
          its worst |error| / (sup|gelu'| a + |z|) over the clip, times that magnitude at the element (the emulation's figure is
          taken over the clip, as norm_reference takes the worst row: a single element's emulation may round exactly by luck);
        bf16 output, VALU: BAR x the emulation's worst |z error| / a times a sup|gelu'|, plus the GELU polynomial's
          2.5e-5 + 1.6e-5 |z| (tests/test_isa_audit.py::test_gelu_poly_error_bound);
        bf16 output, matrix cores: the header's split.  Every operand keeps a bf16 high and low part: v = vh + vl + e with
          |vl| <= 2^-9 |v| and |e| <= 2^-18 |v| (the low part is the rounded residue of the high part's rounding).  Of
          (ah + al + ea)(xh + xl + ex) the kernel keeps ah xh + ah xl + al xh; what is lost is al xl + ea x + a ex <= 3 x 2^-18 |a x|
          (1 + 2^-8).  sh rides as a high / low pair: 2^-18 |sh|.  The 32 products of bf16 pairs are exact in fp32; their sum has at most
          32 links, sc w_j one rounding, sc and sh three: gamma(36).  So |dz| <= (3 x 2^-18 (1 + 2^-8) + gamma(36)) a =: SPLIT a, through
          sup|gelu'|, plus the chord table's 1.1e-5 |z| + 1e-7 (test_conv0_gelu_table_error_bound).  On a waveform with a DC offset
          |sh| ~ |mean| rstd |gamma| is large against z and this bound is wider than a bf16 ulp of the output: a documented property;
     3. the output rounding U_OUT[dtype] |out|.
   Backward.  |dW[c,j] - truth| <= (gamma(chain_bwd) + eps_gelu'[c] + eps_stats[c]) Mag[c,j] gscale + u |dW0 + dW|  (the accumulate).
     chain_bwd: VALU 256 sequential fused multiply-adds of a 256-frame block + 3 (the cast of the fp64 fold, gscale, +=) = 259;
       matrix cores: a block's 8 time tiles x 2 halves x (high + low part of X) x 16 products = 512, + 3 = 515, and the split of X adds
       2^-18, and with bf16 dY dz enters as ONE bf16 operand: + 2^-9 Mag (test_conv0_matrix_core_backward_equals_the_valu_backward).
     eps_gelu'[c] = max_j E_gelu[c,j] / Mag[c,j], E_gelu the Mag expression with |dY| e(z) in the place of |dz|: e the absolute error
       of gelu' -- fp32: 8 u (erf 2.5 u on Phi, |z| phi(z) (2 z^2 + 5) u <= 1.9 u through exp2(-z^2 / 2 log2 e), the sum 1.2 u);
       bf16 VALU: the polynomial's 1.3e-4; matrix cores: the chord table's 3e-5 for |z| <= 4.3, 1.4e-4 beyond
       (test_gelu_grad_poly_error_bound, test_conv0_gelu_grad_table_error_bound).
     eps_stats[c] = max_j E_stats[c,j] / Mag[c,j], E_stats the first-order effect of the moment and statistics allowances on dw_j:
       dz through z (|dY| sup|gelu''| |gamma| (|x_hat| drstd / rstd + rstd dmean), sup|gelu''| = 2 phi(0) < 0.8), S2 through x_hat,
       the three explicit factors rstd (<= 2 (drstd / rstd) Mag: S2 carries the third), (R w - mean M)_j through dR, dM and dmean, and M_j.
     dgamma and dbeta: the same form with their own magnitudes sum_b sum_t |dz x_hat| and sum_b sum_t |dz|.

d. emulate(): a numpy emulation of the documented moment scheme (1024-frame chunks, fp32 partials in the partition above, fp64 fold,
   the documented statistics and dw formulas, the backward's A_j / S1 / S2 as 256 sequential fp32 fused multiply-adds per block).  Not a
   transcription of the kernel.  fault= plants one wrong-kernel behaviour (FAULTS); tests/test_conv0_reference_cpu.py shows which
   allowance each one leaves."""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from tests import elementwise_reference as E
from tests import norm_reference as R

U32, BAR, rnd, gamma, summation_floor, U_OUT = R.U32, R.BAR, R.rnd, E.gamma, R.summation_floor, E.U_OUT
F32, F64 = np.float32, np.float64
BF, FP = torch.bfloat16, torch.float32
TCM, TCH = 1024, 256          # frames per moment chunk / per apply and backward block
MOMENT_CHAIN = 12
EPS, GSCALE = 1e-5, 0.1
SUP_GELU_GRAD, SUP_GELU_GRAD2 = 1.13, 0.8
GELU_POLY_ABS, GELU_POLY_REL = 2.5e-5, 1.6e-5
GELU_TAB_ABS, GELU_TAB_REL = 1e-7, 1.1e-5
GRAD_F32_ABS, GRAD_POLY_ABS, GRAD_TAB_IN, GRAD_TAB_OUT, GRAD_TAB_EDGE = 8 * U32, 1.3e-4, 3e-5, 1.4e-4, 4.3
SPLIT = 3 * 2.0 ** -18 * (1 + 2.0 ** -8) + gamma(36)
CHAIN_BWD = {"valu": TCH + 3, "mfma": 512 + 3}
FORMS = ("fp32", "bf16_valu", "bf16_mfma")
FAULTS = ("drop_chunk_last_frame", "tail_reads_next_clip", "divide_by_L_minus_1", "offdiag_once", "no_var_clamp",
          "mean_in_fp32_before_square")


def form_dtype(form):
    return FP if form == "fp32" else BF


# ---------------------------------------------------------------------------------------------------------------------------
# cases: geometry, waveform families, filters
# ---------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name L k stride r C clips")
ZERO_FILTER = 5                 # channel of the all-zero filter: var = 0 on every clip
EPS_FAMILIES = ("zero", "const")


def _case(L, C, clips, k=10, stride=5, r=3):
    return Case(f"L{L}-k{k}s{stride}-C{C}-{'+'.join(clips)}", L, k, stride, r, C, tuple(clips))


# (the constant clip sits at L = 256: its fp32 sum of squares is exact there while fl(0.7f * 0.7f) < 0.7f^2, so the variance an fp32
#  moment scheme derives is NEGATIVE -- the clamp is exercised)
_PAIRS = {37: ("white", "dc"), 256: ("const", "tone"), 257: ("ar1", "zero"), 1024: ("tone", "dc"), 1025: ("dc", "ar1"),
          1287: ("zeros_ar1", "ar1")}
CASES = [_case(L, C, _PAIRS[L]) for L in sorted(_PAIRS) for C in (32, 128)]
CASES += [_case(37, 8, _PAIRS[37]),
          _case(300, 128, ("ar1", "dc"), k=7, r=2),                     # KW = 10 with padded taps, both matrix-core passes
          _case(1030, 8, ("ar1", "dc"), k=12, stride=4, r=1)]           # KW = 16: VALU only
CASE_IDS = [c.name for c in CASES]


def samples(case):
    return case.stride * (case.L - 1) + case.k + case.r


def eps_dominated(case):
    """bool [B, C]: the (clip, channel) pairs named as eps-dominated -- every channel of an all-zero or constant clip, and the all-zero
    filter's channel on every clip.  True var = 0 there, rstd = eps^-1/2, out = gelu(beta)."""
    m = torch.zeros(len(case.clips), case.C, dtype=torch.bool)
    for b, fam in enumerate(case.clips):
        if fam in EPS_FAMILIES:
            m[b] = True
    m[:, ZERO_FILTER] = True
    return m


def _ar1(n, rng, rho=0.99):
    e = rng.standard_normal(n)
    x = np.empty(n)
    acc = e[0] / math.sqrt(1 - rho * rho)          # stationary start
    x[0] = acc
    for i in range(1, n):
        acc = rho * acc + e[i]
        x[i] = acc
    return x


def _normalised(x):
    """zero mean, unit variance per clip (the recipe's `normalize`)."""
    return (x - x.mean()) / x.std()


def waveform(family, S, stride, seed):
    rng = np.random.default_rng(seed)
    if family == "white":
        x = rng.standard_normal(S)
    elif family == "ar1":
        x = _normalised(_ar1(S, rng))
    elif family == "tone":
        x = _normalised(np.sin(2 * np.pi * 200.0 / 16000.0 * np.arange(S)) + 1e-3 * rng.standard_normal(S))
    elif family == "dc":
        x = 1.0 + 0.01 * rng.standard_normal(S)
    elif family == "zeros_ar1":
        x = np.zeros(S)
        n0 = 1100 * stride
        assert S > n0 + 64
        x[n0:] = _normalised(_ar1(S - n0, rng))
    elif family == "zero":
        x = np.zeros(S)
    elif family == "const":
        x = np.full(S, 0.7)
    else:
        raise ValueError(family)
    return torch.from_numpy(x.astype(F32))


def filters(case, gen):
    """fp32 [C, k]: randn sqrt(2 / k), channels 0..5 the first, second and third difference (centred), the mean filter, a cosine at a
    quarter of the sample rate and the all-zero filter.  A case with a tone clip keeps random filters in the place of the second and
    third difference: those pairings (kappa >= 3e5) have a vacuous variance bound and are deliberately not in the list."""
    C, k = case.C, case.k
    w = torch.randn(C, k, generator=gen) * math.sqrt(2.0 / k)
    c = k // 2
    special = {0: {c - 1: -1.0, c: 1.0}, 1: {c - 1: 1.0, c: -2.0, c + 1: 1.0}, 2: {c - 2: -1.0, c - 1: 3.0, c: -3.0, c + 1: 1.0}}
    for ch, taps in special.items():
        if ch in (1, 2) and "tone" in case.clips:
            continue
        w[ch] = 0
        for j, v in taps.items():
            w[ch, j] = v
    w[3] = 1.0 / k
    w[4] = torch.tensor([math.cos(math.pi / 2 * j) for j in range(k)]).round()
    w[ZERO_FILTER] = 0
    return w.float()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """wav [B, S], w [C, k], gamma, beta, dY fp32 [B, L, C] (round it to the dtype), dW0 / dgamma0 / dbeta0 (the accumulators' seed)."""
    S, B = samples(case), len(case.clips)
    seed = 7919 * case.L + 131 * case.k + case.C
    gen = torch.Generator().manual_seed(seed)
    wav = torch.stack([waveform(f, S, case.stride, seed + 17 * b) for b, f in enumerate(case.clips)])
    w = filters(case, gen)
    g = torch.rand(case.C, generator=gen) + 0.5
    be = 0.1 * torch.randn(case.C, generator=gen)
    dY = 0.3 * torch.randn(B, case.L, case.C, generator=gen)
    seeds = [0.05 * torch.randn(*s, generator=gen) for s in ((case.C, case.k), (case.C,), (case.C,))]
    return SimpleNamespace(wav=wav, w=w, gamma=g, beta=be, dY=dY, dW0=seeds[0], dgamma0=seeds[1], dbeta0=seeds[2])


# ---------------------------------------------------------------------------------------------------------------------------
# a. fp64 truth and b. magnitudes
# ---------------------------------------------------------------------------------------------------------------------------
def forward_truth(wav, w, g, be, k, stride, eps=EPS):
    X = wav.double().unfold(1, k, stride).contiguous()          # [B, L, k]
    B, L, _ = X.shape
    wd, gd, bd = w.double(), g.double(), be.double()
    y = X @ wd.t()                                              # [B, L, C]
    mean = y.sum(1) / L
    d = y - mean[:, None]
    var = (d * d).sum(1) / L
    rstd = 1.0 / torch.sqrt(var + float(F32(eps)))
    xhat = d * rstd[:, None]
    z = xhat * gd + bd
    aX, aw = X.abs(), wd.abs()
    M, aM = X.sum(1), aX.sum(1)                                 # [B, k]
    Rm, aR = X.transpose(1, 2) @ X, aX.transpose(1, 2) @ aX     # [B, k, k]
    T1 = aM @ aw.t() / L
    T2 = torch.einsum("cj,bjk,ck->bc", aw, aR, aw) / L
    kappa = torch.where(var > 0, T2 / var.clamp_min(1e-300), torch.full_like(var, math.inf))
    return SimpleNamespace(X=X, L=L, k=k, stride=stride, eps=float(F32(eps)), w=wd, gamma=gd, beta=bd, y=y, mean=mean, var=var, rstd=rstd, xhat=xhat, z=z,
                           out=R.gelu64(z), M=M, aM=aM, R=Rm, aR=aR, T1=T1, T2=T2, kappa=kappa)


def _mag(t, s1, s2, A):
    """sum_b rstd |gamma| (A_j + s1 |M_j| / L + s2 rstd |(R w - mean M)_j| / L) -> [C, k]; s1, s2 [B, C] and A [B, C, k] magnitudes."""
    Q = torch.einsum("bjk,ck->bcj", t.R, t.w) - t.mean[:, :, None] * t.M[:, None, :]
    per = A + s1[:, :, None] * t.M.abs()[:, None, :] / t.L + (s2 * t.rstd)[:, :, None] * Q.abs() / t.L
    return ((t.rstd * t.gamma.abs())[:, :, None] * per).sum(0)


def _weighted(t, wgt):
    """(sum_t wgt |x_j| [B, C, k], sum_t wgt [B, C], sum_t wgt |x_hat| [B, C]) of a non-negative weight [B, L, C]."""
    return torch.einsum("blc,blj->bcj", wgt, t.X.abs()), wgt.sum(1), (wgt * t.xhat.abs()).sum(1)


def backward_truth(t, dY, gscale=GSCALE, dW0=None, dgamma0=None, dbeta0=None):
    """dW [C, k], dgamma, dbeta (added to the seeds) and the magnitudes of 1b."""
    dy = dY.double()
    dz = dy * R.gelu_grad64(t.z)
    S1, S2 = dz.sum(1), (dz * t.xhat).sum(1)
    dconv = (t.rstd * t.gamma)[:, None] * (dz - S1[:, None] / t.L - t.xhat * S2[:, None] / t.L)
    dW = gscale * torch.einsum("blc,blj->cj", dconv, t.X)
    dgamma, dbeta = gscale * S2.sum(0), gscale * S1.sum(0)
    A, s1, s2 = _weighted(t, dz.abs())
    z0 = torch.zeros((), dtype=torch.float64)
    return SimpleNamespace(dy=dy, dz=dz, S1=S1, S2=S2, gscale=gscale, Mag=_mag(t, S1.abs(), S2.abs(), A), mag_dgamma=s2.sum(0), mag_dbeta=s1.sum(0),
                           dW0=z0 if dW0 is None else dW0.double(), dgamma0=z0 if dgamma0 is None else dgamma0.double(),
                           dbeta0=z0 if dbeta0 is None else dbeta0.double(), dW=dW, dgamma=dgamma, dbeta=dbeta)


# ---------------------------------------------------------------------------------------------------------------------------
# c. allowances
# ---------------------------------------------------------------------------------------------------------------------------
def stats_allowance(t):
    dmean = summation_floor(t.T1, MOMENT_CHAIN) + U32 * t.mean.abs()
    dvar = summation_floor(t.T2 + 2 * t.mean.abs() * t.T1, MOMENT_CHAIN)
    ulp = 2.0 ** -23
    lo = (1 - ulp) / torch.sqrt(t.var + dvar + t.eps)
    hi = (1 + ulp) / torch.sqrt((t.var - dvar).clamp_min(0) + t.eps)
    return SimpleNamespace(dmean=dmean, dvar=dvar, rstd_lo=lo, rstd_hi=hi, drstd=torch.maximum(hi - t.rstd, t.rstd - lo))


def vacuous(t, al, exempt):
    """bool [B, C]: dvar > (var + eps) / 4 outside the named eps-dominated pairs."""
    return (al.dvar > 0.25 * (t.var + t.eps)) & ~exempt


def stats_ratio(t, al, mean_got, rstd_got):
    """(|mean - truth| / dmean, the saved rstd's position in its interval: 1 at either end) [B, C]."""
    rm = (mean_got.double() - t.mean).abs() / al.dmean.clamp_min(1e-300)
    rm = torch.where((al.dmean == 0) & (mean_got.double() == t.mean), torch.zeros_like(rm), rm)
    rs = rstd_got.double()
    rr = torch.where(rs >= t.rstd, (rs - t.rstd) / (al.rstd_hi - t.rstd), (t.rstd - rs) / (t.rstd - al.rstd_lo))
    return rm, rr


def _fma32(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def apply_emulation(t, wav, w, g, be):
    """The documented apply in plain fp32 on the TRUE statistics (rounded to fp32): k fused multiply-adds, one for the affine, erf.
    Returns per clip the worst |z error| / a and the worst |out error| / (sup|gelu'| a + |z|)."""
    X = wav.unfold(1, t.k, t.stride).numpy().astype(F32)
    w32, g32, b32 = w.numpy().astype(F32), g.numpy().astype(F32), be.numpy().astype(F32)
    mu, rs = t.mean.numpy().astype(F32), t.rstd.numpy().astype(F32)
    y = np.zeros(X.shape[:2] + (w32.shape[0],), F32)
    for j in range(t.k):
        y = _fma32(X[:, :, j, None], w32[None, None, :, j], y)
    sc = (rs * g32).astype(F32)
    sh = (b32 - (mu * sc).astype(F32)).astype(F32)
    z = _fma32(y, sc[:, None], sh[:, None])
    zt = torch.from_numpy(z)
    out = 0.5 * zt * (1.0 + torch.erf(zt * 0.7071067811865476))
    a = apply_magnitude(t)
    ez = ((zt.double() - t.z).abs() / a.clamp_min(1e-300)).amax((1, 2))
    eo = ((out.double() - t.out).abs() / (SUP_GELU_GRAD * a + t.z.abs()).clamp_min(1e-300)).amax((1, 2))
    return ez, eo


def apply_magnitude(t):
    """a [B, L, C] = sum_j |sc w_j x_j| + |sh|, sc = rstd gamma, sh = beta - mean sc."""
    sc = t.rstd * t.gamma
    return (t.X.abs() @ t.w.abs().t()) * sc.abs()[:, None] + (t.beta - t.mean * sc).abs()[:, None]


def forward_bound(t, al, form, emu):
    """Per-element bound [B, L, C] on |out - truth| (1c); emu = apply_emulation(...)."""
    ez, eo = emu
    dz_stats = t.gamma.abs() * (t.xhat.abs() * (al.drstd / t.rstd)[:, None] + (t.rstd * al.dmean)[:, None])
    a = apply_magnitude(t)
    if form == "fp32":
        app = BAR * eo[:, None, None] * (SUP_GELU_GRAD * a + t.z.abs())
    elif form == "bf16_valu":
        app = BAR * ez[:, None, None] * a * SUP_GELU_GRAD + GELU_POLY_ABS + GELU_POLY_REL * t.z.abs()
    else:
        app = SPLIT * a * SUP_GELU_GRAD + GELU_TAB_ABS + GELU_TAB_REL * t.z.abs()
    return dz_stats * SUP_GELU_GRAD + app + U_OUT[form_dtype(form)] * t.out.abs()


def gelu_grad_error(t, form):
    """Absolute error bound of the form's gelu' at every element [B, L, C]."""
    if form == "fp32":
        return torch.full_like(t.z, GRAD_F32_ABS)
    if form == "bf16_valu":
        return torch.full_like(t.z, GRAD_POLY_ABS)
    return torch.where(t.z.abs() <= GRAD_TAB_EDGE, torch.full_like(t.z, GRAD_TAB_IN), torch.full_like(t.z, GRAD_TAB_OUT))


def backward_bounds(t, bw, al, form, bwd_mfma):
    """Bounds on |dW|, |dgamma|, |dbeta| errors ([C, k], [C], [C]) for the accumulated results (1c)."""
    chain = CHAIN_BWD["mfma" if bwd_mfma else "valu"]
    base = gamma(chain) + ((2.0 ** -18 + 2.0 ** -9) if bwd_mfma else 0.0)
    ady = bw.dy.abs()
    # eps_gelu': the Mag expression with |dY| e(z) in the place of |dz|
    wg = ady * gelu_grad_error(t, form)
    Ag, s1g, s2g = _weighted(t, wg)
    E_gelu = _mag(t, s1g, s2g, Ag)
    # eps_stats: first-order effect of the moment and statistics allowances
    rel_rs = al.drstd / t.rstd                                                      # [B, C]
    dxhat = t.xhat.abs() * rel_rs[:, None] + (t.rstd * al.dmean)[:, None]           # [B, L, C]
    wz = ady * SUP_GELU_GRAD2 * t.gamma.abs() * dxhat                               # |d dz|
    Az, s1z, s2z = _weighted(t, wz)
    dS2 = s2z + (bw.dz.abs() * dxhat).sum(1)                                        # through dz and through x_hat
    E_dz = _mag(t, s1z, dS2, Az)
    Adz, s1dz, s2dz = _weighted(t, bw.dz.abs())
    per_clip_mag = _PerClip(t, bw.S1.abs(), bw.S2.abs(), Adz)
    dM = summation_floor(t.aM, MOMENT_CHAIN)                                        # [B, k]
    dRw = summation_floor(torch.einsum("bjk,ck->bcj", t.aR, t.w.abs()), MOMENT_CHAIN)   # [B, C, k]
    dQ = dRw + t.mean.abs()[:, :, None] * dM[:, None, :] + al.dmean[:, :, None] * t.M.abs()[:, None, :]
    mom = (bw.S1.abs()[:, :, None] * dM[:, None, :] + (bw.S2.abs() * t.rstd)[:, :, None] * dQ) / t.L
    E_stats = E_dz + (2 * rel_rs[:, :, None] * per_clip_mag).sum(0) + ((t.rstd * t.gamma.abs())[:, :, None] * mom).sum(0)
    safe = bw.Mag.clamp_min(1e-300)
    live = bw.Mag > 0
    eps_gelu = torch.where(live, E_gelu / safe, torch.zeros_like(safe)).amax(1)
    eps_stats = torch.where(live, E_stats / safe, torch.zeros_like(safe)).amax(1)
    bW = (base + eps_gelu + eps_stats)[:, None] * bw.Mag * bw.gscale + U32 * (bw.dW0 + bw.dW).abs()

    def scalar(mag, e_gelu, e_stats, seed, val):
        sm = mag.clamp_min(1e-300)
        eg = torch.where(mag > 0, e_gelu / sm, torch.zeros_like(sm))
        es = torch.where(mag > 0, e_stats / sm, torch.zeros_like(sm))
        return (base + eg + es) * mag * bw.gscale + U32 * (seed + val).abs()
    bG = scalar(bw.mag_dgamma, s2g.sum(0), dS2.sum(0) + (rel_rs * s2dz).sum(0), bw.dgamma0, bw.dgamma)
    bB = scalar(bw.mag_dbeta, s1g.sum(0), s1z.sum(0), bw.dbeta0, bw.dbeta)
    return SimpleNamespace(dW=bW, dgamma=bG, dbeta=bB, eps_gelu=eps_gelu, eps_stats=eps_stats)


def _PerClip(t, s1, s2, A):
    """The Mag expression before the sum over clips [B, C, k]."""
    Q = torch.einsum("bjk,ck->bcj", t.R, t.w) - t.mean[:, :, None] * t.M[:, None, :]
    per = A + s1[:, :, None] * t.M.abs()[:, None, :] / t.L + (s2 * t.rstd)[:, :, None] * Q.abs() / t.L
    return (t.rstd * t.gamma.abs())[:, :, None] * per


def ratio(err, bound):
    """Worst |err| / bound; an error where the bound is zero counts as infinite, NaN as infinite."""
    err, bound = err.double().abs().reshape(-1), bound.double().reshape(-1)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return r.max().item() if r.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# d. numpy emulation of the documented scheme
# ---------------------------------------------------------------------------------------------------------------------------
def _chunk_partial(Xc):
    """fp32 partial moments of one chunk (<= 1024 frames, [nt, k]): a thread's 4 frames in order, 6 pairwise wave steps, 2 block adds.
    Returns (M [k], R [k, k])."""
    nt, k = Xc.shape
    pad = np.zeros((TCM, k), F32)
    pad[:nt] = Xc
    a = pad.reshape(4, 256, k)
    m1, m2 = np.zeros((256, k), F32), np.zeros((256, k, k), F32)
    for i in range(4):
        m1 = m1 + a[i]
        m2 = _fma32(a[i][:, :, None], a[i][:, None, :], m2)
    v = np.concatenate([m1, m2.reshape(256, k * k)], 1).reshape(4, 64, -1)
    for _ in range(6):
        v = v[:, 0::2] + v[:, 1::2]
    v = v[:, 0]
    v = (v[0] + v[1]) + (v[2] + v[3])
    return v[:k], v[k:].reshape(k, k)


def emulate(wav, w, g, be, dY, k, stride, L, eps=EPS, gscale=GSCALE, dW0=None, dgamma0=None, dbeta0=None, fault=None):
    """mean, rstd fp32 [B, C], out fp32 [B, L, C]; dW, dgamma, dbeta fp32 (accumulated onto the seeds) of the documented scheme.
    dY None: forward only."""
    assert fault is None or fault in FAULTS
    B, S = wav.shape
    flat = np.concatenate([wav.numpy().astype(F32).reshape(-1), np.zeros(k + stride, F32)])
    w64 = w.numpy().astype(F64)
    C = w64.shape[0]
    idx = np.arange(L)[:, None] * stride + np.arange(k)[None, :]
    Xs, Ms, Rs = [], [], []
    for b in range(B):
        X = flat[b * S + idx]
        Xs.append(X.copy())
        if fault == "tail_reads_next_clip":            # the clip's last frame is taken at the next clip's start
            X = X.copy()
            X[L - 1] = flat[(b + 1) * S:(b + 1) * S + k]
        M, Rm = np.zeros(k, F64), np.zeros((k, k), F64)
        for t0 in range(0, L, TCM):
            nt = min(TCM, L - t0)
            if fault == "drop_chunk_last_frame":
                nt -= 1
            pm, pr = _chunk_partial(X[t0:t0 + nt])
            M += pm.astype(F64)
            Rm += pr.astype(F64)
        Ms.append(M)
        Rs.append(Rm)
    M, Rm = np.stack(Ms), np.stack(Rs)                          # [B, k], [B, k, k] fp64
    Ld = float(L - 1 if fault == "divide_by_L_minus_1" else L)
    s1 = M @ w64.T                                              # [B, C]
    if fault == "offdiag_once":
        up = np.triu(Rm)
        s2 = np.einsum("cj,bjk,ck->bc", w64, up, w64)
    else:
        s2 = np.einsum("cj,bjk,ck->bc", w64, Rm, w64)
    mu = s1 / Ld
    msq = mu.astype(F32).astype(F64) ** 2 if fault == "mean_in_fp32_before_square" else mu * mu
    var = s2 / Ld - msq
    if fault != "no_var_clamp":
        var = np.maximum(var, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = 1.0 / np.sqrt(var + F64(F32(eps)))
    mean32, rstd32 = mu.astype(F32), rs.astype(F32)
    # the apply pass in fp32 on these statistics: k fused multiply-adds, one for the affine, erf
    X = np.stack(Xs)                                            # [B, L, k] fp32
    w32, g32, b32 = w.numpy().astype(F32), g.numpy().astype(F32), be.numpy().astype(F32)
    y = np.zeros((B, L, C), F32)
    for j in range(k):
        y = _fma32(X[:, :, j, None], w32[None, None, :, j], y)
    with np.errstate(invalid="ignore", over="ignore"):
        sc = (rstd32 * g32).astype(F32)
        zf = torch.from_numpy(_fma32(y, sc[:, None], (b32 - (mean32 * sc).astype(F32)).astype(F32)[:, None]))
    res = SimpleNamespace(mean=torch.from_numpy(mean32), rstd=torch.from_numpy(rstd32), out=0.5 * zf * (1.0 + torch.erf(zf * 0.7071067811865476)),
                          dW=None, dgamma=None, dbeta=None)
    if dY is None:
        return res
    # backward: fp32 recompute per frame, 256 sequential fused multiply-adds per block, fp64 fold, the documented formulas
    xh = ((y - mean32[:, None]).astype(F32) * rstd32[:, None]).astype(F32)
    z = _fma32(xh, g32, b32)
    dz = (dY.float() * R.gelu_grad32(torch.from_numpy(z), False)).numpy().astype(F32)
    nch = (L + TCH - 1) // TCH
    pad = nch * TCH - L
    dzp = np.concatenate([dz, np.zeros((B, pad, C), F32)], 1).reshape(B, nch, TCH, C)
    xhp = np.concatenate([xh, np.zeros((B, pad, C), F32)], 1).reshape(B, nch, TCH, C)
    Xp = np.concatenate([X, np.zeros((B, pad, k), F32)], 1).reshape(B, nch, TCH, k)
    A, a1, a2 = np.zeros((B, nch, C, k), F32), np.zeros((B, nch, C), F32), np.zeros((B, nch, C), F32)
    for i in range(TCH):
        a1 = a1 + dzp[:, :, i]
        a2 = _fma32(dzp[:, :, i], xhp[:, :, i], a2)
        A = _fma32(dzp[:, :, i, :, None], Xp[:, :, i, None, :], A)
    A, S1, S2 = A.astype(F64).sum(1), a1.astype(F64).sum(1), a2.astype(F64).sum(1)      # [B, C, k], [B, C]
    mud, rsd, gd = mean32.astype(F64), rstd32.astype(F64), g32.astype(F64)
    Rw = np.einsum("bjk,ck->bcj", Rm, w64)
    acc = (rsd * gd)[:, :, None] * (A - S1[:, :, None] * M[:, None, :] / Ld
                                    - (S2 * rsd)[:, :, None] * (Rw - mud[:, :, None] * M[:, None, :]) / Ld)
    gs = F32(gscale)

    def accumulate(seed, v, shape):
        s0 = np.zeros(shape, F32) if seed is None else seed.numpy().astype(F32)
        return torch.from_numpy((s0 + (gs * v.astype(F32)).astype(F32)).astype(F32))
    res.dW = accumulate(dW0, acc.sum(0), (C, k))
    res.dgamma = accumulate(dgamma0, S2.sum(0), (C,))
    res.dbeta = accumulate(dbeta0, S1.sum(0), (C,))
    return res
