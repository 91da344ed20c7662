"""Plain references of csrc/elementwise.hip (and st5_multi_transpose_bf16 of csrc/optim.hip), the yardsticks
tests/test_elementwise_fp64_gpu.py holds the kernels to.  Written from the entry points' descriptions in include/speecht5_hip.h and the
torch / fairseq call sites they cite, not from the kernels.  Two forms where arithmetic is involved (one function, `emulate`):

- fp64: the truth, explicit formulas in torch double on the already-rounded inputs;
- emulation: the same arithmetic in fp32 with the kernels' rounding points -- exp and log through their base-2 forms where the
  kernels use the fast intrinsics (exp(x) = exp2(x * log2e), log(x) = log2(x) * ln2), the result rounded to the output type.

Data movement (casts, pads, gathers, selects, framing) has one form: the expected array, compared bit for bit.

The dropout counter rule is tests/attention_reference.py's (counter = the element's flat index); the metric, BAR and the gamma_n
bound are tests/norm_reference.py's.  Pinned to torch on the CPU by tests/test_elementwise_reference_cpu.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import attention_reference as A
from tests import norm_reference as R

ACT_NONE, ACT_GELU, ACT_RELU, ACT_TANH, ACT_LRELU_01, ACT_LRELU_001 = 0, 1, 2, 3, 4, 5
ACT_NAMES = {ACT_NONE: "none", ACT_GELU: "gelu", ACT_RELU: "relu", ACT_TANH: "tanh", ACT_LRELU_01: "lrelu0.1", ACT_LRELU_001: "lrelu0.01"}
SLOPE = {ACT_LRELU_01: 0.1, ACT_LRELU_001: 0.01}
TRANSCENDENTAL = (ACT_GELU, ACT_TANH)
SE_MASKING, SE_DELTA = 0, 1

U32 = R.U32
U_OUT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}    # unit roundoff of an output type, as the class-B bound counts it
LOG2E_F32 = R.LOG2E_F32
LN2_F32 = np.float32(0.6931471805599453)
FLAT_ROW = 2055           # a flat case shorter than this takes its emulation figure from this long a prefix of the shared values


def gamma(k):
    """gamma_k = k u / (1 - k u), u = 2^-24: k fp32 roundings in a row."""
    return k * U32 / (1 - k * U32)


def rounded(x, dtype):
    return R.rnd(x.float(), dtype)


def _exp32(x):
    """__expf: exp2 of the fp32 product x * log2e."""
    return torch.exp2(x * float(LOG2E_F32))


def _log32(x):
    """__logf: log2(x) times the fp32 ln 2."""
    return torch.log2(x) * float(LN2_F32)


# ---------------------------------------------------------------------------------------------------------------------------
# activations (st5_act_fwd / st5_act_bwd, the act of st5_channel_affine and st5_pad_time_act)
# ---------------------------------------------------------------------------------------------------------------------------
def act(a, x, emulate=False):
    """act(x): fp64 of the fp32 / bf16 values in x, or the fp32 emulation (not yet rounded to the output type)."""
    z = x.float() if emulate else x.double()
    if a == ACT_NONE:
        return z
    if a == ACT_GELU:     # erf form (torch F.gelu default; fairseq gelu)
        return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))
    if a == ACT_RELU:     # torch.relu: NaN stays NaN
        return torch.where(z <= 0, torch.zeros_like(z), z)
    if a == ACT_TANH:
        return torch.tanh(z)
    if a in SLOPE:
        s = float(np.float32(SLOPE[a])) if emulate else SLOPE[a]
        return torch.where(z > 0, z, z * s)
    raise ValueError(a)


def act_grad(a, x, emulate=False):
    """d act / dx at the pre-activation x."""
    z = x.float() if emulate else x.double()
    if a == ACT_NONE:
        return torch.ones_like(z)
    if a == ACT_GELU:
        cdf = 0.5 * (1.0 + torch.erf(z * 0.7071067811865476))
        e = _exp32(-0.5 * z * z) if emulate else torch.exp(-0.5 * z * z)
        return cdf + z * (0.3989422804014327 * e)
    if a == ACT_RELU:
        return (z > 0).to(z.dtype)
    if a == ACT_TANH:
        t = torch.tanh(z)
        return 1.0 - t * t
    if a in SLOPE:
        s = float(np.float32(SLOPE[a])) if emulate else SLOPE[a]
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, s))
    raise ValueError(a)


def act_fwd(a, x, dtype=None, emulate=False):
    y = act(a, x, emulate)
    return rounded(y, dtype) if emulate else y


def act_bwd(a, dy, x, dtype=None, emulate=False):
    g = (dy.float() if emulate else dy.double()) * act_grad(a, x, emulate)
    return rounded(g, dtype) if emulate else g


def act_roundings(a, backward=False):
    """k of the class-B bound for the rounding-bounded activations: ReLU forward moves bits (0); ReLU backward is one product by 0 or 1
    (exact, counted 1); LeakyReLU: the fp32 slope constant and the product (2)."""
    if a in (ACT_NONE, ACT_RELU):
        return 1 if backward else 0
    assert a in SLOPE
    return 2


# ---------------------------------------------------------------------------------------------------------------------------
# flat arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def axpby(x, y, a, b):
    """(a x + b y, |a x| + |b y|) in fp64 with the fp32 values of a and b.  k = 3: two products and a sum."""
    a, b = float(np.float32(a)), float(np.float32(b))
    return a * x.double() + b * y.double(), (a * x.double()).abs() + (b * y.double()).abs()


def dropout_keep(seed, p, n):
    """Keep set of st5_dropout: the library's counter rule with counter = element index."""
    return torch.from_numpy(A.keep_mask_flat(seed, p, np.arange(n, dtype=np.uint64)))


def dropout(x, keep, p):
    """fp64: x / (1 - p) for survivors (p as fp32), 0 for the rest.  k = 2: the fp32 1 / (1 - p) and the product."""
    return torch.where(keep, x.double() / (1.0 - float(np.float32(p))), torch.zeros((), dtype=torch.float64))


def dropout_bits(x, keep, p, dtype):
    """What the kernel must store: x * (keep ? fp32(1 / (1 - p)) : 0) in fp32, rounded to dtype (a dropped negative is -0)."""
    s = torch.where(keep, torch.tensor(A.inv_keep(p), dtype=torch.float32), torch.zeros((), dtype=torch.float32))
    return (x.float() * s).to(dtype)


def sumsq(x, scale, init=0.0):
    """(init + scale * sum x^2, |init| + |scale| * sum x^2) in fp64."""
    s = float(np.float32(scale)) * (x.double() ** 2).sum().item()
    return init + s, abs(init) + abs(s)


def sumsq_chain(n, aligned=True, pair=False):
    """Longest addition chain of st5_sumsq on n elements.  Aligned: 8 per trip over ceil(n / 8 / threads) trips + 1 tail element;
    unaligned: one per trip; then 6 wave steps + 3 block adds + 1 cast of the fp64 sum of the block partials (+ 1 for an accumulate)
    (+ 1 per term: the square; + 1 more for the pair's x + y)."""
    threads = min(2048, max(1, ((n // 8 + 1 if aligned else n) + 255) // 256)) * 256
    per_thread = 8 * math.ceil(max(n // 8, 1) / threads) + 1 if aligned else math.ceil(max(n, 1) / threads)
    return per_thread + 6 + 3 + 1 + 1 + (1 if pair else 0)


def sigmoid(z, emulate=False):
    return 1.0 / (1.0 + torch.exp(-z))


def se_predict_fwd(mode, x, src, emulate=False):
    """speecht5.py:937-953: masking y = sigmoid(x) * src, delta y = x - src."""
    z, s = (x.float(), src.float()) if emulate else (x.double(), src.double())
    return sigmoid(z) * s if mode == SE_MASKING else z - s


def se_predict_bwd(mode, dy, x, src, emulate=False):
    """autograd of the above with respect to x: dy * src * s * (1 - s); dy."""
    d, z, s = (dy.float(), x.float(), src.float()) if emulate else (dy.double(), x.double(), src.double())
    if mode == SE_DELTA:
        return d
    sg = sigmoid(z)
    return ((d * s) * (1.0 - sg)) * sg


def log10_floor(x, floor, emulate=False):
    """speech_dataset.py logmel: log10(max(x, floor))."""
    z = x.float() if emulate else x.double()
    return torch.log10(torch.clamp(z, min=float(np.float32(floor))))


def stft_magnitude(reim, nbins, ldh):
    """reim [rows, 2 ldh]: real parts in [0, nbins), imaginary in [ldh, ldh + nbins) -> |.| [rows, ldh], pad columns 0.
    k = 4: two squares, a sum, a square root."""
    re, im = reim[:, :nbins].double(), reim[:, ldh:ldh + nbins].double()
    out = torch.zeros(reim.shape[0], ldh, dtype=torch.float64)
    out[:, :nbins] = torch.sqrt(re * re + im * im)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# row operations
# ---------------------------------------------------------------------------------------------------------------------------
def masked_fill_rows(x, mask, v, dtype):
    """x[r, :] = v where mask[r] (apply_hubert_mask): the expected array in dtype, other rows untouched."""
    out = x.clone()
    out[mask.bool()] = v.to(dtype)
    return out


def masked_fill_rows_bwd(dx, mask, dv0=None):
    """(dx with masked rows zeroed, dv = dv0 + sum of the masked rows, sum |.| + |dv0|)."""
    m = mask.bool()
    out = dx.clone()
    out[m] = 0
    t = dx.double()[m]
    dv0 = torch.zeros(dx.shape[1], dtype=torch.float64) if dv0 is None else dv0.double()
    return out, dv0 + t.sum(0), dv0.abs() + t.abs().sum(0)


def fill_chain(rows):
    """masked_fill_rows_bwd: a thread's rows (every 256th, or all of them below 256 row splits) + the row splits added in order + 1."""
    ny = min(rows, 256)
    return math.ceil(rows / ny) + ny + 1


def add_table_rows(x, table, idx, scale):
    """(x + scale * table[idx], |x| + |scale * table[idx]|).  k = 1 (one fused multiply-add)."""
    t = float(np.float32(scale)) * table.double()[idx.long()]
    return x.double() + t, x.double().abs() + t.abs()


def embed_rows(table, tok, pos, pidx, emb_scale, pos_scale):
    """(emb_scale * table[tok] + pos_scale * pos[pidx], sum |terms|).  k = 2."""
    a = float(np.float32(emb_scale)) * table.double()[tok.long()]
    if pos is None:
        return a, a.abs()
    b = float(np.float32(pos_scale)) * pos.double()[pidx.long()]
    return a + b, a.abs() + b.abs()


def scatter_rows(dy, tok, vocab, scale, table0=None, row_w=None, rw_div=1, rw_mod=1):
    """dtable[tok[r]] += scale * w_r * dy[r] over the rows with 0 <= tok[r] < vocab, w_r = row_w[(r / rw_div) % rw_mod]:
    (table, sum |terms| + |table0|) in fp64 by index_add_."""
    rows, cols = dy.shape
    d = dy.double() * float(np.float32(scale))
    if row_w is not None:
        r = torch.arange(rows)
        d = d * row_w.double()[(r // rw_div) % rw_mod][:, None]
    ok = (tok >= 0) & (tok < vocab)
    t0 = torch.zeros(vocab, cols, dtype=torch.float64) if table0 is None else table0.double()
    out = t0.clone().index_add_(0, tok[ok].long(), d[ok])
    mag = t0.abs().index_add_(0, tok[ok].long(), d[ok].abs())
    return out, mag


def longest_run(tok, vocab):
    ok = tok[(tok >= 0) & (tok < vocab)]
    return int(torch.bincount(ok.long(), minlength=1).max().item()) if ok.numel() else 0


def channel_affine(x, a, b, act_id, dtype=None, emulate=False):
    """y[r, c] = act(x[r, c] * a[c] + b[c]); also the terms |x a| + |b|.  k = 1 (+ the activation's)."""
    if emulate:   # one fused multiply-add: the fp64 value rounded once
        pre = (x.double() * a.double() + b.double()).float()
        return rounded(act(act_id, pre, True), dtype)
    pre = x.double() * a.double() + b.double()
    return act(act_id, pre), (x.double() * a.double()).abs() + b.double().abs()


# ---------------------------------------------------------------------------------------------------------------------------
# layout (expected arrays, bit for bit)
# ---------------------------------------------------------------------------------------------------------------------------
def pad_time(src, pad_l, pad_r, live=None):
    """[B, T, C] -> [B, pad_l + T + pad_r, C], zeros around; rows t >= live (clamped to [0, T]) zero as well."""
    s = src
    if live is not None:
        s = src.clone()
        s[:, max(0, min(int(live), src.shape[1])):] = 0
    return F.pad(s.transpose(1, 2), (pad_l, pad_r)).transpose(1, 2).contiguous()


def edge_rows(Tp, head, tail_start):
    """bool [Tp]: the rows st5_zero_time_edges (t < head or t >= tail_start) writes."""
    t = torch.arange(Tp)
    return (t < head) | (t >= tail_start)


def halo_rows(T, pad_l, pad_r):
    return edge_rows(pad_l + T + pad_r, pad_l, pad_l + T)


def gather3_index(A_, B_, C_, sa, sb, sc, off):
    a, b, c = torch.arange(A_)[:, None, None], torch.arange(B_)[None, :, None], torch.arange(C_)[None, None, :]
    return off + a * sa + b * sb + c * sc


def unfold_rows(wav, k, stride, kpad):
    """[B, S] -> [B * L, kpad]: windows of k samples every `stride`, zero columns from k on; L = (S - k) / stride + 1."""
    w = wav.unfold(1, k, stride)
    return F.pad(w, (0, kpad - k)).reshape(-1, kpad).contiguous()


def stft_frames(wav, n_fft, hop):
    """librosa's centred framing: reflect padding of n_fft / 2 at both ends, L = 1 + S / hop frames of n_fft samples."""
    S = wav.shape[-1]
    padded = np.pad(wav.numpy(), [(0, 0)] * (wav.dim() - 1) + [(n_fft // 2, n_fft // 2)], mode="reflect")
    L = 1 + S // hop
    idx = np.arange(L)[:, None] * hop + np.arange(n_fft)[None, :]
    return torch.from_numpy(np.ascontiguousarray(padded[..., idx]))


def select(keep, a, b):
    """LayerDrop's device-side select: keep != 0 (so -0.0 drops) ? b : a, bytes untouched."""
    return b if keep != 0.0 else a


# ---------------------------------------------------------------------------------------------------------------------------
# cross entropy (fairseq label_smoothed_nll_loss, speech_to_text_loss.py:93-110; eps = 0: F.cross_entropy(reduction="sum"))
# ---------------------------------------------------------------------------------------------------------------------------
def cross_entropy(logits, target, eps, ignore_index, grad_scale, dtype=None, emulate=False):
    """logits [rows, V] (already rounded to the compute type), target int [rows]; rows with target < 0 or == ignore_index count
    nothing.  Returns row_loss, row_nll [rows] and dlogits [rows, V] = grad_scale * d(sum of row losses) / dlogits.
    fairseq: nll = -lprob[t], smooth = -sum_c lprob[c], eps_i = eps / (V - 1), loss = (1 - eps - eps_i) nll + eps_i smooth."""
    rows, V = logits.shape
    skip = (target < 0) | (target == ignore_index)
    tgt = torch.where(skip, torch.zeros_like(target), target).long()
    onehot = F.one_hot(tgt, V)
    if not emulate:
        l = logits.double().requires_grad_(True)
        lp = torch.log_softmax(l, -1)
        nll = -lp.gather(1, tgt[:, None])[:, 0]
        smooth = -lp.sum(1)
        eps_i = eps / (V - 1) if V > 1 else 0.0
        loss = (1.0 - eps - eps_i) * nll + eps_i * smooth
        keep = (~skip).double()
        (loss * keep).sum().backward()
        return (loss * keep).detach(), (nll * keep).detach(), l.grad * grad_scale
    f32 = np.float32
    l = logits.float()
    mx = l.max(1, keepdim=True).values
    se = _exp32(l - mx).sum(1, keepdim=True)
    lse = mx + _log32(se)
    nll = (lse - l.gather(1, tgt[:, None]))[:, 0]
    eps_i = float(f32(eps) / f32(V - 1)) if V > 1 else 0.0
    w = float(f32(1.0) - f32(eps) - f32(eps_i))
    smooth = float(V) * lse[:, 0] - l.sum(1)
    loss = w * nll + eps_i * smooth
    p = _exp32(l - lse)
    g = (w * (p - onehot.float()) + eps_i * (float(V) * p - 1.0)) * float(f32(grad_scale))
    keep = (~skip).float()
    return loss * keep, nll * keep, rounded(g * keep[:, None], dtype)


def cross_entropy_terms(logits, target, eps, ignore_index):
    """Per row, sum |terms| of the loss expression (1 - eps - eps_i)(lse - l_t) + eps_i (V lse - sum l) in fp64, 0 on skipped rows;
    and the chain of one row's loss: a lane's ceil(V / 64) classes + 6 wave steps + 8 roundings of the expression itself (the exp's
    argument, exp, log, lse, nll, two products and their sum)."""
    rows, V = logits.shape
    l = logits.double()
    skip = (target < 0) | (target == ignore_index)
    tgt = torch.where(skip, torch.zeros_like(target), target).long()
    lse = torch.logsumexp(l, -1).abs()
    eps_i = eps / (V - 1) if V > 1 else 0.0
    t = abs(1.0 - eps - eps_i) * (lse + l.gather(1, tgt[:, None])[:, 0].abs()) + eps_i * (V * lse + l.abs().sum(1))
    return t * (~skip).double(), (V + 63) // 64 + 6 + 8


# ---------------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------------
def within_b(got, ref, terms, k, dtype):
    """Class B: |got - fp64| <= gamma_k * sum |terms| + u_out * |fp64| on every element.  Returns (ok, worst error / bound)."""
    g, r = got.double().reshape(-1), ref.double().reshape(-1)
    bound = gamma(k) * terms.double().reshape(-1) + U_OUT[dtype] * r.abs()
    err = (g - r).abs()
    bad = ~(err <= bound)      # (NaN fails)
    worst = torch.where(bound > 0, err / bound.clamp(min=1e-300), (err > 0).double() * math.inf).max().item() if g.numel() else 0.0
    return not bool(bad.any()), worst


def within_d(got, ref, abs_sum, chain):
    """Class D: |got - fp64| <= gamma_(chain + 1) * sum |t| (norm_reference.summation_floor) on every element."""
    g = torch.as_tensor(got, dtype=torch.float64).reshape(-1)
    r = torch.as_tensor(ref, dtype=torch.float64).reshape(-1)
    bound = R.summation_floor(torch.as_tensor(abs_sum, dtype=torch.float64).reshape(-1), chain)
    err = (g - r).abs()
    return not bool((~(err <= bound)).any()), (err / bound.clamp(min=1e-300)).max().item() if g.numel() else 0.0


def flat_errors(x, ref, floor_from):
    """Per element: |x - ref| / max(|ref|, 2^-8 * max |floor_from|): norm_reference's row metric on rows of one element."""
    den = torch.clamp(ref.double().abs(), min=2.0 ** -8 * floor_from.double().abs().max().item()).clamp(min=1e-300)
    e = (x.double() - ref.double()).abs()
    return torch.where(e == 0, torch.zeros_like(e), e / den)


def flat_passes(got, ref_full, emu_full, n):
    """Class C for a flat kernel run on the first n of the shared values: every element within BAR x the emulation's worst element over
    the first max(n, FLAT_ROW) values.  (A prefix of one to nine elements has no statistics of its own: an emulation that happens to
    round its single element exactly would set a bar of zero.)  Returns (ok, kernel worst, emulation worst)."""
    m = max(n, FLAT_ROW)
    assert ref_full.numel() >= m and emu_full.numel() >= m
    ref, emu = ref_full.reshape(-1)[:m], emu_full.reshape(-1)[:m]
    if not torch.isfinite(got.double()).all():
        return False, math.inf, flat_errors(emu, ref, ref).max().item()
    ee = flat_errors(emu, ref, ref).max().item()
    ek = flat_errors(got.reshape(-1), ref[:n], ref).max().item()
    return ek <= R.BAR * ee, ek, ee
