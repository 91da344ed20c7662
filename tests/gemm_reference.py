"""Plain reference of the GEMM family (csrc/gemm.hip: st5_gemm, st5_gemm_tn_group), the yardstick tests/test_gemm_fp64_gpu.py holds every
kernel and epilogue of the family to.  One function, `gemm`, takes what st5_gemm_params describes -- FLAT buffers plus operand descriptors,
not pre-sliced matrices -- and comes in two forms:

- fp64 (emulate=False): the truth.  Operands gathered by the addressing formula of include/speecht5_hip.h written as plain index
  arithmetic (`offsets`), then, in double on the dtype-rounded inputs,
      pre = alpha A B^T + bias[z bias_zs + n];  v = DACT ? pre act'(P) : act(pre);  v *= keep / (1 - p);  v += R;  v += beta C_old;
      Cpre = pre;  asum[m] += sum_k A(m, k)
  with the dropout keep mask from attention_reference.keep_mask_flat at the counter z M N + row N + col the header promises.
- emulation (emulate=True): the same arithmetic with the kernels' rounding points -- fp32 accumulation, every epilogue step its own fp32
  operation in the kernels' order (the fast layout's two explicit fmaf: acc * alpha + bias and beta * C_old + x; the slow layout has none),
  the polynomial GELU / GELU' of common.h in bf16 mode on the fast layout and erff otherwise, R / P / C_old read in their storage type,
  C and Cpre rounded once to theirs (fp32 C under OUT_F32).  Split-K and grouped launches compute the same thing: not modelled.
  `fault=` plants one wrong-kernel behaviour (FAULTS); tests/test_gemm_reference_cpu.py shows that every one of them fails the bar.

The bar (`judge`) is per element and owes nothing to the kernel:
      |got - ref64| <= BAR max(|emu - ref64|, ulp_out(ref64) / 2) + summation_floor(S, chain) (+ the documented GELU polynomial bounds)
with S the fp64 sum of absolute terms behind the element and chain = K + the epilogue's operation count (norm_reference.summation_floor:
the bound of an fp32 sum in ANY order, so the MFMA accumulation order need not be the emulation's)."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests import attention_reference as A
from tests import norm_reference as NR

BAR = NR.BAR
F32 = np.float32
ACT_NONE, ACT_GELU, ACT_RELU, ACT_TANH, ACT_LRELU_01, ACT_LRELU_001 = range(6)
A_KSTRIDED, B_KSTRIDED, OUT_F32, DACT = 1, 2, 4, 8
EPILOGUE_OPS = 16        # alpha, bias, activation (counted as 8 operations: erff / tanhf / the Horner chains are a few ulp), dropout, R, beta, store
GELU_LIPSCHITZ = 1.13    # max |gelu'| = 1.1290 (at x = sqrt 2); the other activations have slope <= 1
GELU_POLY_ABS, GELU_POLY_REL, GELU_GRAD_POLY = 2.4e-5, 1.5e-5, 1.2e-4     # common.h: gelu_poly / gelu_grad_poly error bounds

FAULTS = ("a_last_k", "k_tail_poison", "bias_shift", "alpha_after_bias", "r_row", "mask_shift", "mask_no_base", "beta_before_drop",
          "cpre_post", "asum_skip_row", "asum_overwrite")


class Op:
    """st5_operand on a flat CPU tensor `buf` (its storage type), `off` elements in."""

    def __init__(self, buf, ld, off=0, rpb=0, bstride=0, seg=0, seg_stride=0, zs0=0, zs1=0):
        assert buf.dim() == 1
        self.buf, self.ld, self.off, self.rpb, self.bstride, self.seg, self.seg_stride, self.zs0, self.zs1 = \
            buf, ld, off, rpb, bstride, seg, seg_stride, zs0, zs1

    def vec_ok(self):
        """c_class_vec_ok of gemm.hip for one operand (the buffer itself starts 16-byte aligned)."""
        es = self.buf.element_size()
        return (self.off * es) % 16 == 0 and self.ld % 8 == 0 and self.bstride % 8 == 0 and self.zs0 % 8 == 0 and self.zs1 % 8 == 0


def problem(A, B, C, M, N, K, **kw):
    """st5_gemm_params.  A, B, C, R, P, Cpre: Op (or None); bias: fp32 tensor or None; asum: fp32 buffer whose first M elements are the column (asum_buf) or None; seed: below 2^63, or a slot
    (bit 63 set, the address in the low 48 bits) resolved through seed_slots {address: value}."""
    p = SimpleNamespace(A=A, B=B, C=C, M=M, N=N, K=K, R=None, P=None, Cpre=None, bias=None, bias_zs=0, batch=1, zdiv=1, act=ACT_NONE, flags=0,
                        alpha=1.0, beta=0.0, dropout_p=0.0, seed=0, asum=None, seed_slots=None)
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


# ---------------------------------------------------------------------------------------------------------------------------
# addressing (include/speecht5_hip.h, "Generalised operand addressing")
# ---------------------------------------------------------------------------------------------------------------------------
def offsets(op, n_outer, n_inner, z=0, zdiv=1, rpb=None):
    """[n_outer, n_inner] int64 element offsets into op.buf:
    off + (rpb ? (outer / rpb) bstride + (outer % rpb) ld : outer ld) + (seg ? (inner / seg) seg_stride + inner % seg : inner)
        + (z / zdiv) zs0 + (z % zdiv) zs1."""
    rpb = op.rpb if rpb is None else rpb
    o = np.arange(n_outer, dtype=np.int64)
    i = np.arange(n_inner, dtype=np.int64)
    po = (o // rpb) * op.bstride + (o % rpb) * op.ld if rpb else o * op.ld
    pi = (i // op.seg) * op.seg_stride + i % op.seg if op.seg else i
    return op.off + po[:, None] + pi[None, :] + (z // zdiv) * op.zs0 + (z % zdiv) * op.zs1


def gather_ab(op, rows, K, kstrided, z=0, zdiv=1):
    """[rows, K] of an A / B operand: k-major (outer = row, inner = k) or k-strided (outer = k, inner = row)."""
    if kstrided:
        return op.buf[torch.from_numpy(offsets(op, K, rows, z, zdiv))].t()
    return op.buf[torch.from_numpy(offsets(op, rows, K, z, zdiv))]


def c_offsets(op, p, rpb=None):
    """[batch, M, N] offsets of a C-class operand."""
    return np.stack([offsets(op, p.M, p.N, z, p.zdiv, rpb) for z in range(p.batch)])


def gather_c(op, p, rpb=None):
    return op.buf[torch.from_numpy(c_offsets(op, p, rpb))]


# ---------------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------------
_SLOPE = {ACT_LRELU_01: float(F32(0.1)), ACT_LRELU_001: float(F32(0.01))}     # the header's slopes as the kernels hold them (fp32 constants)


def act64(act, x):
    if act == ACT_GELU:
        return NR.gelu64(x)
    if act == ACT_RELU:
        return torch.where(x > 0, x, torch.zeros_like(x))
    if act == ACT_TANH:
        return torch.tanh(x)
    if act in _SLOPE:
        return torch.where(x > 0, x, _SLOPE[act] * x)
    return x


def act_grad64(act, x):
    if act == ACT_GELU:
        return NR.gelu_grad64(x)
    if act == ACT_RELU:
        return (x > 0).to(x.dtype)
    if act == ACT_TANH:
        return 1.0 - torch.tanh(x) ** 2
    if act in _SLOPE:
        return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, _SLOPE[act]))
    return torch.ones_like(x)


def act32(act, x, poly):
    if act == ACT_GELU:
        return NR.gelu32(x, poly)
    return act64(act, x)            # (fp32 tensors in, fp32 out: one rounding per operation)


def act_grad32(act, x, poly):
    if act == ACT_GELU:
        return NR.gelu_grad32(x, poly)
    if act == ACT_TANH:
        t = torch.tanh(x)
        return 1.0 - t * t
    return act_grad64(act, x)


def lipschitz(act):
    return GELU_LIPSCHITZ if act == ACT_GELU else 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------------------------------------------------------
def resolve_seed(p):
    s = int(p.seed)
    return int(p.seed_slots[s & 0x0000FFFFFFFFFFFF]) if s >> 63 else s


def keep_mask(p, fault=None):
    """[batch, M, N] bool: element counter z M N + row N + col."""
    z = np.arange(p.batch, dtype=np.uint64)[:, None, None] * np.uint64(p.M * p.N)
    if fault == "mask_no_base":
        z = z * np.uint64(0)
    idx = z + np.arange(p.M, dtype=np.uint64)[None, :, None] * np.uint64(p.N) + np.arange(p.N, dtype=np.uint64)[None, None, :]
    if fault == "mask_shift":
        idx = idx + np.uint64(1)
    return torch.from_numpy(A.keep_mask_flat(resolve_seed(p), p.dropout_p, idx))


# ---------------------------------------------------------------------------------------------------------------------------
# the operation
# ---------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on fp32 tensors (the product of two fp32 is exact in double)."""
    return (a.double() * b.double() + c.double()).float()


def fast_layout(p):
    """gemm.hip: ea.fast = c_vec_ok && N % 8 == 0 (every present C-class operand readable as 8-element vectors)."""
    return p.N % 8 == 0 and all(o is None or o.vec_ok() for o in (p.C, p.R, p.P, p.Cpre))


def gemm(p, dtype, emulate=False, fault=None):
    """Result of st5_gemm(p, dtype) as [batch, M, N] double tensors (the emulation's already rounded to their storage types):
    C, Cpre (or None), asum [M] (or None), keep (or None); from the fp64 form also S (sum of absolute terms behind C), S_pre (behind Cpre),
    S_asum, chain, and extra (absolute allowance for the GELU polynomials of the bf16 fast layout, else None)."""
    assert fault is None or (emulate and fault in FAULTS), fault
    dt = torch.float32 if emulate else torch.float64
    aks, bks, out_f32, dact = bool(p.flags & A_KSTRIDED), bool(p.flags & B_KSTRIDED), bool(p.flags & OUT_F32), bool(p.flags & DACT)
    c_dtype = torch.float32 if out_f32 else dtype
    alpha, beta = float(F32(p.alpha)), float(F32(p.beta))
    fast = fast_layout(p)
    poly = emulate and dtype == torch.bfloat16 and fast
    Am = torch.stack([gather_ab(p.A, p.M, p.K, aks, z, p.zdiv) for z in range(p.batch)]).to(dt)
    Bm = torch.stack([gather_ab(p.B, p.N, p.K, bks, z, p.zdiv) for z in range(p.batch)]).to(dt)
    if fault == "a_last_k":
        Am[:, p.M // 2, p.K - 1] = 0
    prod = torch.bmm(Am, Bm.transpose(1, 2))
    if fault == "k_tail_poison":                     # one element past K taken into every product (poison 1.0 on both sides)
        prod = prod + 1.0
    bias = None
    if p.bias is not None:
        n = np.arange(p.N)
        if fault == "bias_shift":                    # the last (partial) 8-vector of a row reads the bias one column on
            n = np.where(n >= (p.N - 1) // 8 * 8, np.minimum(n + 1, p.N - 1), n)
        bias = torch.stack([p.bias[z * p.bias_zs + torch.from_numpy(n)] for z in range(p.batch)])[:, None, :].to(dt)
    if bias is None:
        pre = prod * alpha
    elif fault == "alpha_after_bias":
        pre = (prod + bias) * alpha
    elif emulate and fast:
        pre = _fma32(prod, torch.tensor(alpha, dtype=dt), bias)
    else:
        pre = prod * alpha + bias
    Pm = gather_c(p.P, p).to(dt) if dact else None
    if dact:
        v = pre * (act_grad32(p.act, Pm, poly) if emulate else act_grad64(p.act, Pm))
    else:
        v = act32(p.act, pre, poly) if emulate else act64(p.act, pre)
    post = v
    Rm = None
    if p.R is not None:
        Rm = gather_c(p.R, p, rpb=0 if fault == "r_row" else None).to(dt)
    old = gather_c(p.C, p).to(dt) if beta != 0 else None
    keep = None
    scale = None
    if p.dropout_p > 0:
        keep = keep_mask(p)
        scale = keep_mask(p, fault).to(dt) * A.inv_keep(p.dropout_p)
    if fault == "beta_before_drop" and old is not None:
        v = v + beta * old
    if scale is not None:
        v = v * scale
    if Rm is not None:
        v = v + Rm
    if old is not None and fault != "beta_before_drop":
        v = _fma32(torch.tensor(beta, dtype=dt), old, v) if emulate and fast else v + beta * old
    asum = None
    if p.asum is not None:
        assert p.batch == 1
        rows = Am[0] if fault != "asum_skip_row" else Am[0][:, :-1]
        asum = rows.sum(1) if fault == "asum_overwrite" else p.asum[:p.M].to(dt) + rows.sum(1)
    cpre = (post if fault == "cpre_post" else pre) if p.Cpre is not None else None
    out = SimpleNamespace(keep=keep, fast=fast, c_dtype=c_dtype)
    if emulate:
        out.C = NR.rnd(v, c_dtype).double()
        out.Cpre = NR.rnd(cpre, dtype).double() if cpre is not None else None
        out.asum = asum.double() if asum is not None else None
        return out
    out.C, out.Cpre, out.asum = v, cpre, asum
    # sum of absolute terms behind an element: |alpha| sum |a| |b| + |bias|, through the activation's Lipschitz factor and 1 / (1 - p),
    # plus |R| + |beta C_old|
    S_pre = abs(alpha) * torch.bmm(Am.abs(), Bm.abs().transpose(1, 2))
    if bias is not None:
        S_pre = S_pre + bias.abs()
    S = S_pre * lipschitz(p.act)
    extra = None
    if dtype == torch.bfloat16 and fast and p.act == ACT_GELU:
        extra = GELU_GRAD_POLY * pre.abs() if dact else torch.where(pre.abs() <= 4, torch.full_like(pre, GELU_POLY_ABS), GELU_POLY_REL * pre.abs())
    if keep is not None:
        S = S * A.inv_keep(p.dropout_p)
        extra = extra * A.inv_keep(p.dropout_p) if extra is not None else None
    if Rm is not None:
        S = S + Rm.abs()
    if old is not None:
        S = S + (beta * old).abs()
    out.S, out.S_pre, out.extra, out.chain = S, S_pre, extra, p.K + EPILOGUE_OPS
    out.S_asum = Am[0].abs().sum(1) + p.asum[:p.M].double().abs() if p.asum is not None else None
    out.pre_drop = post          # the value a wrong mask bit would add or remove (times 1 / (1 - p))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the bar
# ---------------------------------------------------------------------------------------------------------------------------
def ulp_out(ref, dtype):
    """Spacing of `dtype` (bf16 / fp32) at |ref|, elementwise (double); subnormal spacing below the smallest normal."""
    bits = 7 if dtype == torch.bfloat16 else 23
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - bits)


def bar_terms(ref, emu, S, chain, dtype, extra=None):
    """(den, floor) of the bar, per element: den = max(|emu - ref|, ulp_out(ref) / 2), floor = summation_floor(S, chain) (+ extra)."""
    return torch.maximum((emu - ref).abs(), 0.5 * ulp_out(ref, dtype)), NR.summation_floor(S, chain, extra)


def bar_ratio(got, ref, den, floor):
    """(|got - ref| - floor) / den per element, inf where got is not finite: an element passes <=> its ratio <= BAR.  THE bar: `judge`
    and tests/test_gemm_fp64_gpu.py (on the device) both evaluate it through this function."""
    return torch.nan_to_num(((got - ref).abs() - floor).clamp_min(0) / den, nan=math.inf, posinf=math.inf)


def tolerance(ref, emu, S, chain, dtype, extra=None):
    """Per element: BAR max(|emu - ref|, ulp / 2) + summation_floor(S, chain) (+ extra)."""
    den, floor = bar_terms(ref, emu, S, chain, dtype, extra)
    return BAR * den + floor


def judge(got, ref, emu, S, chain, dtype, extra=None):
    """(ok, kernel worst |error|, emulation worst |error|, worst ratio) with bar_ratio's ratio; ok <=> ratio <= BAR everywhere.
    All tensors double, same shape, same device."""
    den, floor = bar_terms(ref, emu, S, chain, dtype, extra)
    worst = bar_ratio(got, ref, den, floor).max().item()
    return worst <= BAR, torch.nan_to_num((got - ref).abs(), nan=math.inf).max().item(), (emu - ref).abs().max().item(), worst


def mask_decides(ref, tol, p_drop):
    """Share of elements for which a wrong mask bit (an error of |x| / (1 - p), x the value in front of the dropout) would stay below
    8 x the element's tolerance.  The dropout cases' inputs keep this <= 1 %: the comparison by value then decides every mask bit."""
    return ((ref.pre_drop.abs() * A.inv_keep(p_drop)) < 8 * tol).double().mean().item()


# ---------------------------------------------------------------------------------------------------------------------------
# case generators shared by tests/test_gemm_reference_cpu.py and tests/test_gemm_fp64_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------
SLOT_ADDRESS = 0x7F0000001000      # stand-in address of a seed slot on the CPU (the GPU test puts the slot's device address there)
GUARD = 64                 # sentinel elements behind every buffer
NAN = float("nan")
KINDS = ("plain", "bias", "alpha_bias", "gelu_pre", "drop_res", "dact", "beta", "res")
RT_KINDS = ("relu", "tanh", "lrelu01", "lrelu001", "d_relu", "d_tanh", "d_lrelu01", "d_lrelu001", "all", "f32_res")
_ACT_OF = {"relu": ACT_RELU, "tanh": ACT_TANH, "lrelu01": ACT_LRELU_01, "lrelu001": ACT_LRELU_001}


def ceil8(n):
    return (n + 7) // 8 * 8


def make_op(dtype, n_outer, n_inner, values=None, batch=1, zdiv=1, fill=NAN, **desc):
    """An operand in a fresh flat buffer: every element `fill` (NaN: a read outside the operand poisons the result), `values`
    [batch, n_outer, n_inner] scattered through the descriptor, GUARD more elements behind the last one the descriptor reaches."""
    op = Op(torch.empty(0, dtype=dtype), **desc)
    offs = np.stack([offsets(op, n_outer, n_inner, z, zdiv) for z in range(batch)])
    op.buf = torch.full((int(offs.max()) + 1 + GUARD,), fill, dtype=dtype)
    if values is not None:
        op.buf[torch.from_numpy(offs).reshape(-1)] = values.reshape(-1).to(dtype)
    return op


def ab_op(vals, dtype, kstrided, pad=8):
    """A / B matrix [rows, K] as a plain operand whose leading dimension is `pad` elements wider than the matrix (the K tail, or the
    columns beyond the matrix, hold NaN)."""
    rows, K = vals.shape
    if kstrided:
        return make_op(dtype, K, rows, vals.t()[None], ld=ceil8(rows) + pad)
    return make_op(dtype, rows, K, vals[None], ld=ceil8(K) + pad)


def inputs(M, N, K, batch=1, seed=0, bias_offset=0.0):
    """fp32 values of one problem: A ~ 0.5 N(0, 1), B ~ N(0, 1) / sqrt K, bias ~ bias_offset + N(0, 1) (0.5 N(0, 1) around an offset),
    R, P, C0 ~ N(0, 1), asum0 ~ N(0, 1)."""
    g = torch.Generator().manual_seed(1000003 * M + 7919 * N + 31 * K + batch + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(A=r(batch, M, K) * 0.5, B=r(batch, N, K) / math.sqrt(K), bias=r(batch * N) * (0.5 if bias_offset else 1.0) + bias_offset,
                R=r(batch, M, N), P=r(batch, M, N), C0=r(batch, M, N), asum0=r(M))


def c_layout(name, M, N, batch=1, rpb=0, zdiv=1):
    """Descriptor fields of a C-class operand.  plain: rows of ceil8(N) + 8 elements; unaligned: the same one element into the buffer (no
    16-byte vectors: the slow epilogue); rowsplit: blocks of rpb rows with two halo rows behind each.  Batches lie a 24-element gap apart."""
    ld = ceil8(N) + 8
    d = dict(ld=ld, off=1 if name == "unaligned" else 0)
    rows = M
    if name == "rowsplit":
        d.update(rpb=rpb, bstride=(rpb + 2) * ld)
        rows = (M + rpb - 1) // rpb * (rpb + 2)
    if batch > 1:          # (zdiv == batch: z / zdiv = 0 and z % zdiv = z, the batch stride is zs1)
        d.update({"zs0" if zdiv == 1 else "zs1": rows * ld + 24})
    return d


def case(M, N, K, dtype, kind="plain", aks=False, bks=False, layout="plain", rpb=0, batch=1, zdiv=1, b_pad=8, seed=77, slot=False, p_drop=0.1,
         v=None):
    """One st5_gemm problem of epilogue `kind` (KINDS, RT_KINDS) on plain A / B operands; every C-class operand in `layout`.  zdiv: 1 or
    batch (the batch index then reaches the operands through zs1).  slot: the seed is handed over as a seed slot (bit 63 set)."""
    drop = kind in ("drop_res", "all")
    v = v or inputs(M, N, K, batch, bias_offset=3.0 if drop else 0.0)
    out_f32 = kind == "f32_res"
    cd = torch.float32 if out_f32 else dtype
    assert zdiv in (1, batch) and (batch == 1 or not (aks or bks))
    lay = c_layout(layout, M, N, batch, rpb, zdiv)

    def ab(x, ks):
        if batch == 1:
            return ab_op(x[0], dtype, ks, b_pad)
        rows, ld = x.shape[1], ceil8(K) + 8
        return make_op(dtype, rows, K, x, batch, zdiv, ld=ld, **{"zs0" if zdiv == 1 else "zs1": rows * ld + 16})
    kw = dict(flags=(A_KSTRIDED if aks else 0) | (B_KSTRIDED if bks else 0) | (OUT_F32 if out_f32 else 0), batch=batch, zdiv=zdiv)
    c_op = lambda vals, t: make_op(t, M, N, vals, batch, zdiv, **lay)
    if slot:
        seed_kw = dict(seed=(1 << 63) | SLOT_ADDRESS, seed_slots={SLOT_ADDRESS: seed})
    else:
        seed_kw = dict(seed=seed)
    bias = v["bias"].clone()
    bias_kw = dict(bias=bias, bias_zs=N if batch > 1 else 0)
    C = c_op(None, cd)
    if kind == "bias":
        kw.update(bias_kw)
    elif kind == "alpha_bias":
        kw.update(bias_kw, alpha=0.5)
    elif kind == "gelu_pre":
        kw.update(bias_kw, act=ACT_GELU, Cpre=c_op(None, dtype))
    elif kind == "drop_res":
        kw.update(bias_kw, dropout_p=p_drop, **seed_kw, R=c_op(v["R"], cd))
    elif kind == "dact":
        kw.update(P=c_op(v["P"], dtype), act=ACT_GELU, alpha=0.5)
        kw["flags"] |= DACT
    elif kind == "beta":
        C = c_op(v["C0"], cd)
        kw.update(beta=1.0)
    elif kind in ("res", "f32_res"):
        kw.update(R=c_op(v["R"], cd))
    elif kind in _ACT_OF:
        kw.update(bias_kw, act=_ACT_OF[kind])
    elif kind.startswith("d_"):
        kw.update(P=c_op(v["P"], dtype), act=_ACT_OF[kind[2:]])
        kw["flags"] |= DACT
    elif kind == "all":
        C = c_op(v["C0"], cd)
        kw.update(bias_kw, act=ACT_GELU, Cpre=c_op(None, dtype), dropout_p=p_drop, **seed_kw, R=c_op(v["R"], cd), beta=1.0)
    else:
        assert kind == "plain", kind
    return problem(ab(v["A"], aks), ab(v["B"], bks), C, M, N, K, **kw)


def asum_buf(values):
    """The bias-gradient column as the kernel gets it: [0, M) the old contents, GUARD NaN elements behind them that no launch may touch."""
    buf = torch.full((values.numel() + GUARD,), NAN, dtype=torch.float32)
    buf[:values.numel()] = values.float()
    return buf


def wgrad_case(M, N, K, dtype, beta=0.0, asum=False, seed=0):
    """The weight-gradient form: C[M, N] (+)= A^T B with A [K, M], B [K, N] k-strided, fp32 C; asum accumulates onto non-zero contents."""
    v = inputs(M, N, K, seed=seed)
    C = make_op(torch.float32, M, N, v["C0"][None] if beta else None, ld=ceil8(N) + 8)
    return problem(ab_op(v["A"][0], dtype, True), ab_op(v["B"][0], dtype, True), C, M, N, K, flags=A_KSTRIDED | B_KSTRIDED | OUT_F32, beta=beta,
                   asum=asum_buf(v["asum0"]) if asum else None)


def drop_cases(dtype):
    """(name, problem) of the dropout-addressing cases: batch = 3 through zs1 (zdiv = 3) and zs0 (zdiv = 1), row-split C and R
    (rpb = 50, two halo rows), seed direct and through a slot, p = 0.1 and 0.5; N = 136 on the fast layout and, with unaligned operands, on the
    slow one (aligned counters), N = 83 and 100 on the slow layout with unaligned counters (63 * 83 is odd: so is every other batch's base)."""
    out = []
    for N, layout in ((136, "plain"), (136, "unaligned"), (83, "plain"), (100, "plain")):
        tag = f"N={N} {layout}"
        out.append((f"{tag} batch=3 zdiv=3 p=0.1", case(63, N, 128, dtype, "drop_res", layout=layout, batch=3, zdiv=3, p_drop=0.1, seed=1234567)))
        out.append((f"{tag} batch=3 zdiv=1 p=0.5 slot", case(63, N, 128, dtype, "drop_res", layout=layout, batch=3, zdiv=1, p_drop=0.5, seed=2 ** 40 + 5, slot=True)))
        if layout == "plain":
            out.append((f"{tag} rpb=50 p=0.5", case(200, N, 128, dtype, "drop_res", layout="rowsplit", rpb=50, p_drop=0.5, seed=99)))
            out.append((f"{tag} rpb=50 p=0.1 slot", case(200, N, 128, dtype, "drop_res", layout="rowsplit", rpb=50, p_drop=0.1, seed=3, slot=True)))
    return out


# shapes of tests/test_gemm_fp64_gpu.py (here so that the CPU test can sweep the same lists)
GEN_MS, GEN_NS, GEN_KS = (1, 63, 128, 200, 257), (8, 72, 83, 100, 136, 264), (8, 24, 64, 136, 300)
UNALIGNED_SHAPES = ((63, 72, 24), (200, 136, 136), (257, 264, 300))
TILE_MS, TILE_NS, TILE_KS = (1, 63, 200, 257, 520), (8, 72, 136, 264, 520), (128, 192, 320, 448)
FIRST256_FP32_SHAPES = ((1, 8, 64), (63, 72, 96), (200, 136, 160), (257, 264, 224), (520, 520, 64))      # 2, 3, 5, 7 k-tiles of 32
RT_GENERAL_SHAPES, RT_TILE_SHAPE = ((200, 136, 136), (63, 83, 24)), {torch.bfloat16: (200, 136, 320), torch.float32: (200, 136, 160)}
ROWSPLIT_RPBS, ROWSPLIT_N, ROWSPLIT_K = (49, 100), 136, 192


def rowsplit_case(dtype, kind, rpb):
    """A, C and every other C-class operand split every rpb rows (A with three, the others with two halo rows behind each block)."""
    M, N, K = 4 * rpb, ROWSPLIT_N, ROWSPLIT_K
    v = inputs(M, N, K, bias_offset=3.0 if kind == "drop_res" else 0.0)
    p = case(M, N, K, dtype, kind, layout="rowsplit", rpb=rpb, v=v)
    lda = ceil8(K) + 8
    p.A = make_op(dtype, M, K, v["A"], ld=lda, rpb=rpb, bstride=(rpb + 3) * lda)
    return p


def all_dropout_problems(dtype):
    """(name, problem) of EVERY problem with dropout that tests/test_gemm_fp64_gpu.py runs in `dtype` (one per set of values: the
    operand forms and tile kernels of a shape share them)."""
    yield from drop_cases(dtype)
    for M in GEN_MS:
        for N in GEN_NS:
            for K in GEN_KS:
                yield f"general {M}x{N}x{K}", case(M, N, K, dtype, "drop_res")
    for M, N, K in UNALIGNED_SHAPES:
        yield f"unaligned {M}x{N}x{K}", case(M, N, K, dtype, "drop_res", layout="unaligned")
    if dtype == torch.bfloat16:
        for M in TILE_MS:
            for N in TILE_NS:
                for K in TILE_KS:
                    yield f"tile {M}x{N}x{K}", case(M, N, K, dtype, "drop_res")
    else:
        for M, N, K in FIRST256_FP32_SHAPES:
            yield f"first256 {M}x{N}x{K}", case(M, N, K, dtype, "drop_res")
    for M, N, K in RT_GENERAL_SHAPES + (RT_TILE_SHAPE[dtype],):
        yield f"run-time all {M}x{N}x{K}", case(M, N, K, dtype, "all")
    for rpb in ROWSPLIT_RPBS:
        yield f"rowsplit rpb={rpb}", rowsplit_case(dtype, "drop_res", rpb)
