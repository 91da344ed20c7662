"""csrc/elementwise.hip (and st5_multi_transpose_bf16 of csrc/optim.hip) through the C ABI against the references of
tests/elementwise_reference.py, at the smallest shapes that reach every path: scalar tails (n % 8 != 0), several blocks, the second
trip of every grid-stride loop (grids are capped at 2048 blocks: 4 194 304 elements for the 8-wide kernels, 2 097 152 for se_predict,
524 288 for the one-element-per-thread kernels), the second trip of a lane's column loop (cols > 64; > 512 for add_table_rows), last
blocks with fewer than 4 live rows, the rows > 256 partial-sum path of masked_fill_rows_bwd, base pointers 1 and 3 elements off a
16-byte boundary (the scalar path of the flat entry points; one such case per entry point is long enough for the second trip of
that path's one-element-per-thread loop, n > 524 288), and NaN / +-inf through the activations.

Bars -- nothing in a bar comes from a kernel's output.
A  exact: every data movement (casts included: round-to-nearest-even of the same fp32 value) is compared bit for bit.
B  |kernel - fp64| <= gamma_k sum |terms| + u_out |fp64|, k = the fp32 roundings of the kernel's expression, written at each case:
   axpby 3 (two products, a sum); add_table_rows 1 (one fma); embed_rows 2 (product, fma); channel_affine 1 (fma) + the activation's;
   ReLU forward 0, ReLU backward 1, LeakyReLU 2 (the fp32 slope, the product); dropout survivors 2 (fp32 1 / (1 - p), the product);
   se_predict delta 1; gather3 accumulate 1; stft_magnitude 4 (two squares, a sum, a root).  u_out = 2^-24 (fp32), 2^-8 (bf16).
C  transcendental (GELU, tanh forward and backward, se_predict masking, log10_floor, channel_affine with GELU / tanh, cross entropy):
   worst row of ||kernel - fp64|| / max(||fp64 row||, 2^-8 largest row norm) <= BAR = 4 x the same for the fp32 emulation
   (norm_reference.passes).  A flat kernel's rows are single elements, and the emulation's figure is taken over the first
   max(n, 2055) of the values the case's n are a prefix of (elementwise_reference.flat_passes).  With bf16 outputs the rounding to the
   8-bit significand dominates kernel and emulation alike (every bf16 ratio is 1.000): those cases pin rounding, range and indexing, but
   could not tell a slightly wrong transcendental from a right one -- only the fp32 cases discriminate there.
D  reductions: |kernel - fp64| <= gamma_(n + 1) sum |t| (+ |initial value|), n = the longest addition chain:
   sumsq / sumsq_pair   8 x trips + 1 tail + 6 wave steps + 3 block adds + 1 cast (+ 1 accumulate, + 1 the pair's x + y); unaligned:
                        1 x trips instead of 8 x trips + 1 (elementwise_reference.sumsq_chain);
   masked_fill dv       ceil(rows / 256) rows of a thread + min(rows, 256) partials in order + 1 (fill_chain);
   atomic scatter       the most frequent id's count + 1;
   deterministic scatter  32 rows of a piece + ceil(rows / 32) chunks of a run + 2 (scale, accumulate);
   cross entropy        the atomic sums: a row's ceil(V / 64) + 6 + 8 (cross_entropy_terms) + rows.
   The row losses of the _rows form are class C; only the atomic sums are judged here.
   Run-to-run bit equality is asserted for the deterministic forms (sumsq, sumsq_pair, masked_fill dv, the deterministic scatter).

Every output is followed (and, at an offset base, preceded) by a sentinel guard region that must come back bit-identical; buffers a
kernel only partly writes are pre-filled with sentinels and everything outside the specified region must be untouched; everything
runs under util.poisoned_allocations(); one pass per case.  The measured class-C ratios of an MI355X run are in
profiles/elementwise_fp64_ratios.txt."""
import functools
import math
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from speecht5_amd import hip
from tests import elementwise_reference as E
from tests import norm_reference as R
from tests.util import poisoned_allocations

pytestmark = pytest.mark.gpu

BF, FP, I32 = torch.bfloat16, torch.float32, torch.int32
DTYPES = [BF, FP]
IDS = ["bf16", "fp32"]
SENT = -7.25                 # exact in bf16
SENT_I = 0x5A5A5A5A
GUARD = 4096
FRONT = 8                    # elements in front of an aligned base: 16 bytes of bf16, 32 of fp32
ERR_ARG, ERR_ALIGN = 1, 2

BIG8 = 4194304 + 2 * 2048 + 3          # second grid-stride trip of the 8-wide kernels, with a tail
BIG_SE = 2097152 + 1027                # ... of se_predict
MULTI = 256 * 8 * 3 + 5                # several blocks, no stride
FLAT_N = [1, 7, 8, 9, 2055, MULTI]
FLAT_CASES = [(n, 0) for n in FLAT_N + [BIG8]] + [(2055, 1), (2055, 3), (BIG8, 1)]      # (BIG8, 1): the scalar path's second grid-stride trip
SE_CASES = [(n, 0) for n in FLAT_N + [BIG_SE]] + [(2055, 1), (2055, 3), (BIG_SE, 1)]
ACTS = [E.ACT_GELU, E.ACT_RELU, E.ACT_TANH, E.ACT_LRELU_01, E.ACT_LRELU_001]


@pytest.fixture(autouse=True)
def _poisoned_and_settled():
    """Every test runs under poisoned allocations and starts with no recorded miss; whatever a test recorded and did not raise itself
    (it ended early on a hard assert, or forgot settle()) is raised here."""
    _missed.clear()
    with poisoned_allocations():
        yield
    settle()


def name(dtype):
    return {BF: "bf16", FP: "fp32", I32: "i32"}[dtype]


class Buf:
    """A device buffer of `shape` whose first element lies `off` elements past a 16-byte boundary, sentinels in front and GUARD
    sentinels behind.  init: None = NaN (-1 for integers), "sent" = sentinels, or a host tensor."""

    def __init__(self, shape, dtype, dev, off=0, init=None):
        self.shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        self.n, self.dtype = int(np.prod(self.shape)), dtype
        self.sent = SENT if dtype.is_floating_point else SENT_I
        self.flat = torch.full((FRONT + off + self.n + GUARD,), self.sent, dtype=dtype, device=dev)
        assert self.flat.data_ptr() % 16 == 0
        self.lo = FRONT + off
        self.t = self.flat[self.lo:self.lo + self.n]
        if init is None:
            self.t.fill_(float("nan") if dtype.is_floating_point else -1)
        elif not isinstance(init, str):
            self.t.copy_(init.reshape(-1).to(dtype))
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == (off * self.flat.element_size()) % 16

    def cpu(self):
        return self.t.cpu().view(self.shape)

    def intact(self, what=""):
        assert bool(torch.all(self.flat[:self.lo] == self.sent)) and bool(torch.all(self.flat[self.lo + self.n:] == self.sent)), \
            f"guard region of {what or 'an output'} overwritten"


def sync_intact(*bufs):
    torch.cuda.synchronize()
    for k, b in enumerate(bufs):
        b.intact(f"output {k}")


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    eq = bits(a) == bits(b)
    assert bool(eq.all()), f"{what}: {int((~eq).sum())} of {eq.numel()} elements differ, first at {int((~eq).reshape(-1).nonzero()[0])}"


@functools.lru_cache(maxsize=None)
def vals(seed, n=BIG8, scale=3.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def vals_dt(seed, dtype, scale=3.0):
    """The shared values rounded to `dtype` (as fp32): every flat case's n is a prefix."""
    return R.rnd(vals(seed, BIG8, scale), dtype)


def span(n):
    """How much of the shared values a flat case of n elements needs references of."""
    return max(n, E.FLAT_ROW)


_missed = []


def report(family, case, nm, ek, ee):
    print(f"elementwise fp64 pin: {family} | {case} | {nm} | kernel {ek:.3e} emulation {ee:.3e} ratio {ek / ee if ee > 0 else (0.0 if ek == 0 else math.inf):.3f}")


def hold_c(family, case, nm, res):
    ok, ek, ee = res
    report(family, case, nm, ek, ee)
    if not ok:
        _missed.append(f"{family} {case} {nm}: kernel {ek:.3e}, emulation {ee:.3e} (bar {R.BAR} x)")


def hold_b(what, got, ref, terms, k, dtype):
    ok, worst = E.within_b(got, ref, terms, k, dtype)
    if not ok:
        _missed.append(f"{what}: class B bound (k = {k}) missed, worst error / bound {worst:.3f}")


def hold_d(what, got, ref, abs_sum, chain):
    ok, worst = E.within_d(got, ref, abs_sum, chain)
    if not ok:
        _missed.append(f"{what}: class D bound (chain {chain}) missed, worst error / bound {worst:.3f}")


def settle():
    missed = list(_missed)
    assert not missed, "; ".join(missed)


def call(fn, *args):
    hip.check(getattr(hip.lib(), fn)(*args), fn)


# ---- flat kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,off", FLAT_CASES)
def test_casts(cuda, n, off, dtype):
    """Class A: fp32 -> dtype rounds to nearest even, dtype -> fp32 is exact; the same at an offset base."""
    x = vals(0)[:n]
    src, dst = Buf(n, FP, cuda, off, x), Buf(n, dtype, cuda, off)
    call("st5_cast_from_f32", src.ptr, dst.ptr, 1, n, 0, hip.dt(dtype), hip.stream())
    sync_intact(dst)
    same_bits(dst.cpu(), x.to(dtype), "cast_from_f32")
    back = Buf(n, FP, cuda, off)
    call("st5_cast_to_f32", dst.ptr, back.ptr, n, hip.dt(dtype), hip.stream())
    sync_intact(back)
    same_bits(back.cpu(), x.to(dtype).float(), "cast_to_f32")
    if off:     # only one side off the boundary takes the scalar path too
        dst2 = Buf(n, dtype, cuda, 0)
        call("st5_cast_from_f32", src.ptr, dst2.ptr, n, 1, 0, hip.dt(dtype), hip.stream())
        sync_intact(dst2)
        same_bits(dst2.cpu(), x.to(dtype), "cast_from_f32, unaligned source only")


def run_act(cuda, a, n, off, dtype, inplace=False):
    x, dy = vals_dt(0, dtype)[:n], vals_dt(1, dtype, 1.0)[:n]
    X, DY = Buf(n, dtype, cuda, off, x), Buf(n, dtype, cuda, off, dy)
    Y = Buf(n, dtype, cuda, off, x) if inplace else Buf(n, dtype, cuda, off)
    call("st5_act_fwd", Y.ptr if inplace else X.ptr, Y.ptr, n, a, hip.dt(dtype), hip.stream())
    DX = Buf(n, dtype, cuda, off)
    call("st5_act_bwd", DY.ptr, X.ptr, DX.ptr, n, a, hip.dt(dtype), hip.stream())
    sync_intact(Y, DX, X, DY)
    same_bits(X.cpu(), x.to(dtype), "act: input changed")
    return Y.cpu(), DX.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,off", FLAT_CASES)
def test_activations(cuda, n, off, dtype):
    """All five activations forward and backward.  GELU and tanh: class C; ReLU and LeakyReLU: class B (k = 0 / 1 / 2).  At an
    offset base: the same bits as at the aligned one, also in place (what st5_pad_time_act's fallback does)."""
    m = span(n)
    x, dy = vals_dt(0, dtype)[:m], vals_dt(1, dtype, 1.0)[:m]
    for a in ACTS:
        case = f"n={n} off={off} {name(dtype)}"
        y, dx = run_act(cuda, a, n, off, dtype)
        if a in E.TRANSCENDENTAL:
            hold_c("act_fwd " + E.ACT_NAMES[a], case, "y", E.flat_passes(y.float(), E.act_fwd(a, x), E.act_fwd(a, x, dtype, True), n))
            hold_c("act_bwd " + E.ACT_NAMES[a], case, "dx", E.flat_passes(dx.float(), E.act_bwd(a, dy, x), E.act_bwd(a, dy, x, dtype, True), n))
        else:
            ref, rb = E.act_fwd(a, x[:n]), E.act_bwd(a, dy[:n], x[:n])
            hold_b(f"act_fwd {E.ACT_NAMES[a]} {case}", y, ref, ref.abs(), E.act_roundings(a), dtype)
            hold_b(f"act_bwd {E.ACT_NAMES[a]} {case}", dx, rb, rb.abs(), E.act_roundings(a, True), dtype)
        if off:
            y0, dx0 = run_act(cuda, a, n, 0, dtype)
            same_bits(y, y0, f"act_fwd {E.ACT_NAMES[a]}: offset {off} against aligned")
            same_bits(dx, dx0, f"act_bwd {E.ACT_NAMES[a]}: offset {off} against aligned")
            same_bits(run_act(cuda, a, n, off, dtype, inplace=True)[0], y0, f"act_fwd {E.ACT_NAMES[a]} in place at offset {off}")
    settle()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_activations_nonfinite(cuda, dtype):
    """A NaN comes out of every activation's forward as NaN (vector body and scalar tail); +-inf through ReLU, LeakyReLU and tanh
    gives torch's values.  (GELU at +-inf is not asserted.)"""
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([nan, inf, -inf, -0.0, 0.0, 1.5, -2.5, nan, inf, -inf, nan], dtype=torch.float32)     # 8 in the body, 3 in the tail
    torch_act = {E.ACT_GELU: F.gelu, E.ACT_RELU: torch.relu, E.ACT_TANH: torch.tanh, E.ACT_LRELU_01: lambda z: F.leaky_relu(z, 0.1),
                 E.ACT_LRELU_001: lambda z: F.leaky_relu(z, 0.01), E.ACT_NONE: lambda z: z}
    for off in (0, 1):
        for a in ACTS + [E.ACT_NONE]:
            X, Y = Buf(x.numel(), dtype, cuda, off, x), Buf(x.numel(), dtype, cuda, off)
            call("st5_act_fwd", X.ptr, Y.ptr, x.numel(), a, hip.dt(dtype), hip.stream())
            sync_intact(Y)
            y = Y.cpu().float()
            assert bool(torch.isnan(y[torch.isnan(x)]).all()), f"{E.ACT_NAMES[a]} {name(dtype)} off={off}: NaN swallowed: {y.tolist()}"
            if a != E.ACT_GELU:
                want = torch_act[a](x.to(dtype).float()).to(dtype).float()
                fin = ~torch.isnan(x)
                assert torch.equal(y[fin], want[fin]), f"{E.ACT_NAMES[a]} {name(dtype)} off={off}: {y.tolist()} != {want.tolist()}"


def run_axpby(cuda, n, off, dtype, a, b):
    X, Y = Buf(n, dtype, cuda, off, vals_dt(0, dtype)[:n]), Buf(n, dtype, cuda, off, vals_dt(1, dtype)[:n])
    call("st5_axpby", X.ptr, Y.ptr, n, a, b, hip.dt(dtype), hip.stream())
    sync_intact(Y, X)
    return Y.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,off", FLAT_CASES)
def test_axpby_in_place(cuda, n, off, dtype):
    """y = a x + b y in place, class B with k = 3."""
    y = run_axpby(cuda, n, off, dtype, 0.3, -1.7)
    ref, terms = E.axpby(vals_dt(0, dtype)[:n], vals_dt(1, dtype)[:n], 0.3, -1.7)
    hold_b(f"axpby n={n} off={off}", y, ref, terms, 3, dtype)
    if off:
        same_bits(y, run_axpby(cuda, n, 0, dtype, 0.3, -1.7), f"axpby: offset {off} against aligned")
    settle()


def run_dropout(cuda, n, off, dtype, p, seed, x):
    X, Y = Buf(n, dtype, cuda, off, x), Buf(n, dtype, cuda, off)
    call("st5_dropout", X.ptr, Y.ptr, n, p, seed, hip.dt(dtype), hip.stream())
    sync_intact(Y, X)
    return Y.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,off", FLAT_CASES)
def test_dropout_keep_set_is_the_counter_rule(cuda, n, off, dtype):
    """The keep set equals the counter rule (counter = element index) on every element, tail elements and elements past 2^22
    included; survivors are x / (1 - p) under class B with k = 2, and exactly x * fp32(1 / (1 - p)) rounded once."""
    p, seed = 0.25, 77
    x = vals_dt(0, dtype)[:n].clone()
    x[x == 0] = 1.0
    y = run_dropout(cuda, n, off, dtype, p, seed, x)
    keep = E.dropout_keep(seed, p, n)
    got_keep = y.float() != 0
    assert torch.equal(got_keep, keep), f"keep set differs on {int((got_keep != keep).sum())} of {n} elements, first at {int((got_keep != keep).nonzero()[0])}"
    ref = E.dropout(x, keep, p)
    hold_b(f"dropout n={n} off={off}", y, ref, ref.abs(), 2, dtype)
    same_bits(y, E.dropout_bits(x, keep, p, dtype), "dropout: x * scale rounded once")
    if off:
        same_bits(y, run_dropout(cuda, n, 0, dtype, p, seed, x), f"dropout: offset {off} against aligned")
    settle()


def run_sumsq(cuda, X, n, dtype, scale, acc, init, Y=None):
    out = Buf(1, FP, cuda, 0, torch.tensor([init]))
    if Y is None:
        call("st5_sumsq", X.ptr, out.ptr, n, scale, acc, hip.dt(dtype), hip.stream())
    else:
        call("st5_sumsq_pair", X.ptr, Y.ptr, out.ptr, n, scale, acc, hip.stream())
    sync_intact(out)
    return out.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,off", FLAT_CASES)
def test_sumsq_and_pair(cuda, n, off, dtype):
    """Class D.  out = scale * sum x^2, or out += with accumulate; two calls give the same bits; sumsq_pair(x, y) is sumsq(x + y) bit
    for bit (fp32, same alignment)."""
    x = vals_dt(0, dtype)[:n]
    X = Buf(n, dtype, cuda, off, x)
    chain = E.sumsq_chain(n, aligned=off == 0)
    got = run_sumsq(cuda, X, n, dtype, 0.5, 0, 123.0)          # overwrite: the initial value must not matter
    ref, mag = E.sumsq(x, 0.5)
    hold_d(f"sumsq n={n} off={off}", got, ref, mag, chain)
    same_bits(got, run_sumsq(cuda, X, n, dtype, 0.5, 0, -5.0), "sumsq: second call")
    acc = run_sumsq(cuda, X, n, dtype, 0.25, 1, 3.0)
    ref, mag = E.sumsq(x, 0.25, 3.0)
    hold_d(f"sumsq accumulate n={n} off={off}", acc, ref, mag, chain + 1)
    if dtype == FP:
        y = vals_dt(1, FP)[:n]
        Y = Buf(n, FP, cuda, off, y)
        Z = Buf(n, FP, cuda, off, "sent")
        torch.add(X.t, Y.t, out=Z.t)                            # x + y rounded once, as the pair kernel forms it
        sync_intact(Z)
        assert torch.equal(Z.cpu(), x + y)
        for scale, accf, init in ((0.5, 0, 9.0), (0.25, 1, 3.0)):
            pair = run_sumsq(cuda, X, n, FP, scale, accf, init, Y=Y)
            same_bits(pair, run_sumsq(cuda, Z, n, FP, scale, accf, init), f"sumsq_pair(x, y) against sumsq(x + y), accumulate={accf}")
            same_bits(pair, run_sumsq(cuda, X, n, FP, scale, accf, init, Y=Y), "sumsq_pair: second call")
            ref, mag = E.sumsq((x + y), scale, init if accf else 0.0)
            hold_d(f"sumsq_pair n={n} off={off} accumulate={accf}", pair, ref, mag, E.sumsq_chain(n, aligned=off == 0, pair=True) + accf)
    settle()


def run_se(cuda, n, off, mode):
    xa, xb, src = vals(2)[:n], vals(3)[:n], vals(4, BIG8, 1.0)[:n]
    da, db = vals(5, BIG8, 1.0)[:n], vals(6, BIG8, 1.0)[:n]
    XA, XB, S, DA, DB = (Buf(n, FP, cuda, off, t) for t in (xa, xb, src, da, db))
    YA, YB, GA, GB = (Buf(n, FP, cuda, off) for _ in range(4))
    call("st5_se_predict_fwd", XA.ptr, XB.ptr, S.ptr, YA.ptr, YB.ptr, n, mode, hip.stream())
    call("st5_se_predict_bwd", DA.ptr, DB.ptr, XA.ptr, XB.ptr, S.ptr, GA.ptr, GB.ptr, n, mode, hip.stream())
    sync_intact(YA, YB, GA, GB)
    return YA.cpu(), YB.cpu(), GA.cpu(), GB.cpu()


@pytest.mark.parametrize("mode", [E.SE_MASKING, E.SE_DELTA], ids=["masking", "delta"])
@pytest.mark.parametrize("n,off", SE_CASES)
def test_se_predict(cuda, n, off, mode):
    """masking: class C; delta: class B with k = 1 forward, the gradient handed through bit for bit."""
    got = run_se(cuda, n, off, mode)
    m = span(n)
    src = vals(4, BIG8, 1.0)[:m]
    for k, (xs, ds, nm) in enumerate(((2, 5, "before"), (3, 6, "after"))):
        x, d = vals(xs)[:m], vals(ds, BIG8, 1.0)[:m]
        case = f"n={n} off={off}"
        if mode == E.SE_MASKING:
            hold_c("se_predict_fwd masking", case, nm, E.flat_passes(got[k], E.se_predict_fwd(mode, x, src), E.se_predict_fwd(mode, x, src, True), n))
            hold_c("se_predict_bwd masking", case, nm, E.flat_passes(got[2 + k], E.se_predict_bwd(mode, d, x, src), E.se_predict_bwd(mode, d, x, src, True), n))
        else:
            hold_b(f"se_predict delta {nm} {case}", got[k], E.se_predict_fwd(mode, x[:n], src[:n]), x[:n].abs() + src[:n].abs(), 1, FP)
            same_bits(got[2 + k], d[:n], f"se_predict delta backward {nm}")
    if off:
        for g, g0, nm in zip(got, run_se(cuda, n, 0, mode), ("y before", "y after", "g before", "g after")):
            same_bits(g, g0, f"se_predict {nm}: offset {off} against aligned")
    settle()


# ---- transposes ------------------------------------------------------------------------------------------------------------------
EDGES = [1, 31, 32, 33, 63, 64, 65, 130]
PAIRS = [(1, 31), (31, 1), (32, 33), (33, 32), (63, 65), (65, 63), (64, 130), (130, 64), (1, 130), (130, 1), (31, 64), (64, 32), (33, 63), (65, 130)]


def transpose_table(cuda, jobs):
    """Job table of st5_multi_transpose_bf16 built with the helper the weight images use.  jobs: (src_off, dst_off, rows, cols)."""
    from speecht5_amd import functional as Fn
    tb = Fn._JobTable("elementwise pin", cuda, Fn._Bf16Mirror.JOB)
    for so, do, r, c in jobs:
        tb.append(lambda tile0, so=so, do=do, r=r, c=c: struct.pack(Fn._Bf16Mirror.JOB, so, do, r, c, tile0, 0), ((r + 63) // 64) * ((c + 63) // 64))
    tb.upload()
    return tb


@pytest.mark.parametrize("rows,cols", PAIRS)
def test_transposes(cuda, rows, cols):
    """Class A: st5_cast_from_f32 with transpose in both dtypes and a one-job st5_multi_transpose_bf16."""
    x = vals(7)[:rows * cols].view(rows, cols)
    src = Buf((rows, cols), FP, cuda, 0, x)
    for dtype in DTYPES:
        dst = Buf((cols, rows), dtype, cuda, 0)
        call("st5_cast_from_f32", src.ptr, dst.ptr, rows, cols, 1, hip.dt(dtype), hip.stream())
        sync_intact(dst)
        same_bits(dst.cpu(), x.t().contiguous().to(dtype), f"cast_from_f32 transpose {name(dtype)}")
    sb, db = Buf((rows, cols), BF, cuda, 0, x), Buf((cols, rows), BF, cuda, 0)
    tb = transpose_table(cuda, [(0, 0, rows, cols)])
    addr, njobs, ntiles = tb.launch_args()
    call("st5_multi_transpose_bf16", sb.ptr, db.ptr, addr, njobs, ntiles, hip.stream())
    sync_intact(db)
    same_bits(db.cpu(), x.to(BF).t().contiguous(), "multi_transpose, one job")


def test_multi_transpose_several_jobs(cuda):
    """One launch over five jobs of different shapes (1, 2, 6, 3 and 1 tiles), so the binary search over tile0 goes both ways."""
    shapes = [(1, 33), (31, 65), (130, 65), (64, 130), (63, 1)]
    jobs, so, do = [], 0, 5              # (the copies start off a 16-byte boundary: the kernel moves single elements)
    for r, c in shapes:
        jobs.append((so, do, r, c))
        so, do = so + r * c + 3, do + r * c + 1
    x = vals(8)[:so]
    sb, db = Buf(so, BF, cuda, 0, x), Buf(do, BF, cuda, 0, "sent")
    tb = transpose_table(cuda, jobs)
    addr, njobs, ntiles = tb.launch_args()
    assert njobs == len(shapes) and ntiles == 13
    call("st5_multi_transpose_bf16", sb.ptr, db.ptr, addr, njobs, ntiles, hip.stream())
    sync_intact(db)
    want = torch.full((do,), SENT, dtype=BF)
    for (s0, d0, r, c) in jobs:
        want[d0:d0 + r * c] = x[s0:s0 + r * c].to(BF).view(r, c).t().reshape(-1)
    same_bits(db.cpu(), want, "multi_transpose, five jobs")


# ---- row kernels -----------------------------------------------------------------------------------------------------------------
ROWS = [1, 3, 4, 5, 261]
COLS = [1, 63, 64, 65, 200]


def gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 7919 ** k for k, s in enumerate(seed)) + 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_fill_and_embedding_rows(cuda, rows, cols, dtype):
    """masked_fill_rows (A, unmasked rows untouched), embed_rows with and without positions (B, k = 2), embed_rows_bwd (D)."""
    g = gen(rows, cols)
    d, s = hip.dt(dtype), hip.stream()
    mask = (torch.rand(rows, generator=g) < 0.5).to(torch.uint8)
    mask[-1] = 1
    v = torch.randn(cols, generator=g)
    X = Buf((rows, cols), dtype, cuda, 0, "sent")
    MK, V = mask.to(cuda), v.to(cuda)
    call("st5_masked_fill_rows", X.ptr, MK.data_ptr(), V.data_ptr(), rows, cols, d, s)
    sync_intact(X)
    same_bits(X.cpu(), E.masked_fill_rows(torch.full((rows, cols), SENT, dtype=dtype), mask, v, dtype), "masked_fill_rows")
    vocab, npos = 11, 50
    table, pos = torch.randn(vocab, cols, generator=g), torch.randn(npos, cols, generator=g)
    tok = torch.randint(0, vocab, (rows,), generator=g, dtype=I32)
    pidx = torch.randint(0, npos, (rows,), generator=g, dtype=I32)
    TB, PS, TK, PI = table.to(cuda), pos.to(cuda), tok.to(cuda), pidx.to(cuda)
    for with_pos in (True, False):
        Y = Buf((rows, cols), dtype, cuda, 0)
        call("st5_embed_rows", TB.data_ptr(), TK.data_ptr(), PS.data_ptr() if with_pos else 0, PI.data_ptr() if with_pos else 0, Y.ptr, rows, cols,
             1.7, 0.3, d, s)
        sync_intact(Y)
        ref, terms = E.embed_rows(table, tok, pos if with_pos else None, pidx, 1.7, 0.3)
        hold_b(f"embed_rows {rows}x{cols} pos={with_pos}", Y.cpu(), ref, terms, 2, dtype)
    dy = R.rnd(torch.randn(rows, cols, generator=g), dtype)
    t0 = torch.randn(vocab, cols, generator=g)
    DY, DT = Buf((rows, cols), dtype, cuda, 0, dy), Buf((vocab, cols), FP, cuda, 0, t0)
    call("st5_embed_rows_bwd", DY.ptr, TK.data_ptr(), DT.ptr, rows, cols, 0.6, d, s)
    sync_intact(DT)
    ref, mag = E.scatter_rows(dy, tok, vocab, 0.6, t0)
    hold_d(f"embed_rows_bwd {rows}x{cols}", DT.cpu(), ref, mag, E.longest_run(tok, vocab) + 1)
    settle()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_padded_copies_and_row_zeroing(cuda, rows, cols, dtype):
    """Class A.  pad_time and pad_time_live (B x Tp = `rows` physical rows without padding, 2 x (rows + 3) with it), zero_time_edges
    (nothing outside the edge rows written; head = 0, tail_start = Tp writes nothing), zero_rows_live (fp32)."""
    g = gen(rows, cols, 1)
    d, s = hip.dt(dtype), hip.stream()
    for B, pl, pr in ((1, 0, 0), (2, 2, 1)):
        T, Tp = rows, pl + rows + pr
        src = torch.randn(B, T, cols, generator=g).to(dtype)
        S = Buf((B, T, cols), dtype, cuda, 0, src)
        D = Buf((B, Tp, cols), dtype, cuda, 0)
        call("st5_pad_time", S.ptr, D.ptr, B, T, cols, pl, pr, d, s)
        sync_intact(D)
        same_bits(D.cpu(), E.pad_time(src, pl, pr), f"pad_time B={B} pads=({pl},{pr})")
        for live in (-3, 0, T // 2, T, T + 5):
            cell = torch.tensor([live], dtype=I32, device=cuda)
            D = Buf((B, Tp, cols), dtype, cuda, 0)
            call("st5_pad_time_live", S.ptr, D.ptr, B, T, cols, pl, pr, cell.data_ptr(), d, s)
            sync_intact(D)
            same_bits(D.cpu(), E.pad_time(src, pl, pr, live=live), f"pad_time_live B={B} pads=({pl},{pr}) live={live}")
        for head, tail_start in ((pl, pl + T), (0, Tp), (Tp, Tp), (0, 0), (1 if Tp > 1 else 0, Tp)):
            X = Buf((B, Tp, cols), dtype, cuda, 0, "sent")
            call("st5_zero_time_edges", X.ptr, B, Tp, cols, head, tail_start, d, s)
            sync_intact(X)
            want = torch.full((B, Tp, cols), SENT, dtype=dtype)
            want[:, E.edge_rows(Tp, head, tail_start)] = 0
            same_bits(X.cpu(), want, f"zero_time_edges B={B} Tp={Tp} head={head} tail_start={tail_start}")
        if dtype == FP:
            for live in (-3, 0, Tp // 2, Tp, Tp + 5):
                cell = torch.tensor([live], dtype=I32, device=cuda)
                X = Buf((B, Tp, cols), FP, cuda, 0, "sent")
                call("st5_zero_rows_live", X.ptr, B, Tp, cols, cell.data_ptr(), s)
                sync_intact(X)
                want = torch.full((B, Tp, cols), SENT)
                want[:, max(0, min(live, Tp)):] = 0
                same_bits(X.cpu(), want, f"zero_rows_live B={B} Lx={Tp} live={live}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cols", [8, 504, 512, 520, 1032])
@pytest.mark.parametrize("rows", ROWS)
def test_add_table_rows(cuda, rows, cols, dtype):
    """Class B with k = 1 (one fused multiply-add); the scale read from device memory gives the same bits as the scale by value."""
    g = gen(rows, cols, 2)
    d, s = hip.dt(dtype), hip.stream()
    x = R.rnd(torch.randn(rows, cols, generator=g), dtype)
    table = torch.randn(23, cols, generator=g)
    idx = torch.randint(0, 23, (rows,), generator=g, dtype=I32)
    X, TB, IX = Buf((rows, cols), dtype, cuda, 0, x), table.to(cuda), idx.to(cuda)
    Y, Yd = Buf((rows, cols), dtype, cuda, 0), Buf((rows, cols), dtype, cuda, 0)
    sd = torch.tensor([0.37], device=cuda)
    call("st5_add_table_rows", X.ptr, TB.data_ptr(), IX.data_ptr(), Y.ptr, rows, cols, 0.37, d, s)
    call("st5_add_table_rows_dev", X.ptr, TB.data_ptr(), IX.data_ptr(), Yd.ptr, rows, cols, sd.data_ptr(), d, s)
    sync_intact(Y, Yd)
    ref, terms = E.add_table_rows(x, table, idx, 0.37)
    hold_b(f"add_table_rows {rows}x{cols}", Y.cpu(), ref, terms, 1, dtype)
    same_bits(Yd.cpu(), Y.cpu(), "add_table_rows_dev against the by-value form")
    settle()


def test_row_kernel_argument_errors(cuda):
    L, s = hip.lib(), hip.stream()
    X, Y = Buf((4, 12), FP, cuda, 0, "sent"), Buf((4, 12), FP, cuda, 0, "sent")
    T, IX, SD = torch.zeros(4, 12, device=cuda), torch.zeros(4, dtype=I32, device=cuda), torch.ones(1, device=cuda)
    assert L.st5_add_table_rows(X.ptr, T.data_ptr(), IX.data_ptr(), Y.ptr, 4, 12, 1.0, hip.dt(FP), s) == ERR_ARG
    assert L.st5_add_table_rows_dev(X.ptr, T.data_ptr(), IX.data_ptr(), Y.ptr, 4, 12, SD.data_ptr(), hip.dt(FP), s) == ERR_ARG
    D = Buf((4, 6), FP, cuda, 0, "sent")
    assert L.st5_embed_rows_bwd_det_w(X.ptr, IX.data_ptr(), D.ptr, 4, 6, 4, 1.0, 0, 1, 1, hip.dt(FP), s) == ERR_ARG
    W, O = torch.zeros(2, 9, device=cuda), Buf((2, 16), FP, cuda, 0, "sent")
    assert L.st5_unfold_rows(W.data_ptr(), O.ptr, 2, 9, 10, 5, 16, hip.dt(FP), s) == ERR_ARG
    sync_intact(X, Y, D, O)
    for b in (Y, D, O):
        assert bool(torch.all(b.t == SENT))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cols", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 700])
def test_masked_fill_rows_bwd(cuda, rows, cols, dtype):
    """dx: masked rows zeroed, the others untouched (A); dv += the masked rows' sum (D, fill_chain), without dv, onto zeros and onto
    a non-zero dv; two calls give the same bits."""
    g = gen(rows, cols, 3)
    d, s = hip.dt(dtype), hip.stream()
    dx = R.rnd(torch.randn(rows, cols, generator=g), dtype)
    mask = (torch.rand(rows, generator=g) < 0.5).to(torch.uint8)
    mask[rows // 2] = 1
    MK = mask.to(cuda)
    last = None
    for dv0 in (None, torch.zeros(cols), torch.randn(cols, generator=g), "again"):
        if isinstance(dv0, str):
            dv0 = prev
        prev = dv0
        DX = Buf((rows, cols), dtype, cuda, 0, dx)
        DV = Buf(cols, FP, cuda, 0, dv0) if dv0 is not None else None
        call("st5_masked_fill_rows_bwd", DX.ptr, MK.data_ptr(), DV.ptr if DV else 0, rows, cols, d, s)
        sync_intact(*([DX] + ([DV] if DV else [])))
        want_dx, ref, mag = E.masked_fill_rows_bwd(dx, mask, dv0)
        same_bits(DX.cpu(), want_dx.to(dtype), f"masked_fill_rows_bwd dx (dv {'absent' if dv0 is None else 'given'})")
        if DV:
            hold_d(f"masked_fill_rows_bwd dv {rows}x{cols}", DV.cpu(), ref, mag, E.fill_chain(rows))
            if last is not None and last[0] is dv0:
                same_bits(DV.cpu(), last[1], "masked_fill_rows_bwd dv: second call")
            last = (dv0, DV.cpu())
    settle()


# ---- deterministic scatter ---------------------------------------------------------------------------------------------------------
def scatter_ids(pattern, rows, vocab, g):
    if pattern == "equal":                 # one run over every chunk (more than 8 chunks from 289 rows on: the combine loop's second batch)
        return torch.full((rows,), 7, dtype=I32)
    if pattern == "distinct":
        return torch.randperm(rows, generator=g).to(I32)
    if pattern == "runs":                  # runs of exactly 32 and 64 that end on chunk borders of the sorted order
        ids, k = [], 0
        while len(ids) < rows:
            ids += [k] * (32 if k % 2 == 0 else 64)
            k += 1
        ids = torch.tensor(ids[:rows], dtype=I32)
        return ids[torch.randperm(rows, generator=g)]
    if pattern == "midchunk":              # a run from the middle of chunk 0 to the middle of chunk 3 of the sorted order
        head = min(16, rows)
        run = min(100, rows - head)
        ids = list(range(head)) + [20] * run + [21 + i for i in range(rows - head - run)]
        return torch.tensor(ids, dtype=I32)[torch.randperm(rows, generator=g)]
    assert pattern == "invalid"            # ids < 0 and >= vocab mixed in
    return torch.randint(-3, 9, (rows,), generator=g, dtype=I32).where(torch.rand(rows, generator=g) < 0.7,
                                                                        torch.randint(vocab, vocab + 5, (rows,), generator=g, dtype=I32))


def scatter_det(cuda, DY, TK, t0, rows, cols, vocab, scale, RW, div, mod, dtype):
    DT = Buf((vocab, cols), FP, cuda, 0, t0)
    call("st5_embed_rows_bwd_det_w", DY.ptr, TK.data_ptr(), DT.ptr, rows, cols, vocab, scale, RW.data_ptr() if RW is not None else 0, div, mod,
         hip.dt(dtype), hip.stream())
    sync_intact(DT)
    return DT.cpu()


@pytest.mark.parametrize("cols", [4, 252, 256, 260, 768])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 2047, 2048, 2049, 4100])
def test_deterministic_scatter(cuda, rows, cols):
    """embed_rows_bwd_det_w onto a non-zero table, with and without row weights, both dtypes, five id patterns: class D with
    n = 32 + ceil(rows / 32) + 2; two calls give the same bits; ids outside [0, vocab) contribute nothing and nothing outside the
    table is written."""
    g = gen(rows, cols, 4)
    vocab = rows + 32
    chain = 32 + (rows + 31) // 32 + 2
    rw = torch.rand(3, generator=g) + 0.5
    RW = rw.to(cuda)
    for k, pattern in enumerate(("equal", "distinct", "runs", "midchunk", "invalid")):
        tok = scatter_ids(pattern, rows, vocab, g)
        TK = tok.to(cuda)
        for dt in DTYPES:
            dy = R.rnd(torch.randn(rows, cols, generator=g), dt)
            t0 = torch.randn(vocab, cols, generator=g)
            DY = Buf((rows, cols), dt, cuda, 0, dy)
            for weights in (False, True):
                args = (RW, 4, 3) if weights else (None, 1, 1)
                got = scatter_det(cuda, DY, TK, t0, rows, cols, vocab, 0.6, *args, dt)
                ref, mag = E.scatter_rows(dy, tok, vocab, 0.6, t0, rw if weights else None, args[1], args[2])
                hold_d(f"scatter {pattern} {rows}x{cols} {name(dt)} weights={weights}", got, ref, mag, chain)
                same_bits(got, scatter_det(cuda, DY, TK, t0, rows, cols, vocab, 0.6, *args, dt), f"scatter {pattern}: second call")
    settle()


# ---- layout kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("A_,B_,C_", [(3, 7, 5), (64, 1031, 8)])
def test_gather3(cuda, A_, B_, C_, dtype):
    """A permutation and a tap flip (negative stride, non-zero off); overwrite: class A; accumulate: class B with k = 1.  The second
    shape has 527 872 elements: past the 524 288 of one grid."""
    n = A_ * B_ * C_
    src = vals(9)[:n]
    S = Buf(n, FP, cuda, 0, src)
    d0 = vals_dt(1, dtype, 1.0)[:n].view(A_, B_, C_)
    for nm, (sa, sb, sc, off) in (("permute", (B_, 1, A_ * B_, 0)), ("flip", (B_ * C_, C_, -1, C_ - 1))):
        idx = E.gather3_index(A_, B_, C_, sa, sb, sc, off)
        assert int(idx.min()) == 0 and int(idx.max()) == n - 1 and idx.unique().numel() == n
        D = Buf((A_, B_, C_), dtype, cuda, 0)
        call("st5_gather3", S.ptr, D.ptr, A_, B_, C_, sa, sb, sc, off, 0, hip.dt(dtype), hip.stream())
        sync_intact(D)
        same_bits(D.cpu(), src[idx].to(dtype), f"gather3 {nm}")
        D = Buf((A_, B_, C_), dtype, cuda, 0, d0)
        call("st5_gather3", S.ptr, D.ptr, A_, B_, C_, sa, sb, sc, off, 1, hip.dt(dtype), hip.stream())
        sync_intact(D)
        hold_b(f"gather3 {nm} accumulate", D.cpu(), d0.double() + src[idx].double(), d0.double().abs() + src[idx].double().abs(), 1, dtype)
    settle()


def run_pad_act(cuda, src, pl, pr, a, dtype, src_off=0, dst_off=0):
    B, T, C = src.shape
    S, D = Buf((B, T, C), dtype, cuda, src_off, src), Buf((B, pl + T + pr, C), dtype, cuda, dst_off)
    call("st5_pad_time_act", S.ptr, D.ptr, B, T, C, pl, pr, a, hip.dt(dtype), hip.stream())
    sync_intact(D)
    return D.cpu()


@pytest.mark.parametrize("a", [E.ACT_NONE, E.ACT_LRELU_01], ids=["none", "lrelu"])
@pytest.mark.parametrize("pl,pr", [(0, 0), (3, 0), (0, 2), (5, 5)])
@pytest.mark.parametrize("dtype,C", [(BF, 8), (BF, 12), (FP, 4), (FP, 6)], ids=["bf16-vec", "bf16-rows", "fp32-vec", "fp32-rows"])
def test_pad_time_act(cuda, dtype, C, pl, pr, a):
    """The vector path (16-byte rows) and the fallback (odd rows, or a base off the boundary): halo exact zeros, no activation: class
    A, LeakyReLU: class B with k = 2; the fallback, forced by an unaligned dst or src, gives the vector path's bits."""
    B, T = 2, 9
    src = R.rnd(torch.randn(B, T, C, generator=gen(C, pl, pr)), dtype)
    got = run_pad_act(cuda, src.to(dtype), pl, pr, a, dtype)
    halo = E.halo_rows(T, pl, pr)
    assert bool(torch.all(bits(got[:, halo]) == 0)), "pad_time_act: halo rows are not exact zeros"
    if a == E.ACT_NONE:
        same_bits(got, E.pad_time(src.to(dtype), pl, pr), "pad_time_act without activation")
    else:
        ref = E.act_fwd(a, src)
        hold_b("pad_time_act lrelu", got[:, ~halo], ref, ref.abs(), E.act_roundings(a), dtype)
    same_bits(run_pad_act(cuda, src.to(dtype), pl, pr, a, dtype, dst_off=1), got, "pad_time_act: fallback (unaligned dst) against aligned")
    same_bits(run_pad_act(cuda, src.to(dtype), pl, pr, a, dtype, src_off=3), got, "pad_time_act: fallback (unaligned src) against aligned")
    settle()


def test_pad_time_act_past_one_grid(cuda):
    """bf16, C = 8: 2 x 262 205 rows of one vector each, past the 524 288 threads of one grid."""
    B, T, C, pl, pr = 2, 262200, 8, 3, 2
    src = vals_dt(0, BF)[:B * T * C].view(B, T, C)
    got = run_pad_act(cuda, src.to(BF), pl, pr, E.ACT_LRELU_01, BF)
    halo = E.halo_rows(T, pl, pr)
    assert bool(torch.all(bits(got[:, halo]) == 0))
    ref = E.act_fwd(E.ACT_LRELU_01, src)
    hold_b("pad_time_act lrelu, large", got[:, ~halo], ref, ref.abs(), 2, BF)
    settle()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,T,C,pl,pr", [(3, 7, 5, 0, 0), (3, 7, 5, 3, 0), (3, 7, 5, 0, 2), (3, 7, 5, 5, 5), (1, 1, 1, 1, 1), (2, 3, 26300, 5, 5)])
def test_zero_halo(cuda, B, T, C, pl, pr, dtype):
    """Class A: halo rows exact zeros, the interior untouched (the last shape: 526 000 halo elements, past one grid)."""
    Tp = pl + T + pr
    X = Buf((B, Tp, C), dtype, cuda, 0, "sent")
    call("st5_zero_halo", X.ptr, B, T, C, pl, pr, hip.dt(dtype), hip.stream())
    sync_intact(X)
    want = torch.full((B, Tp, C), SENT, dtype=dtype)
    want[:, E.halo_rows(T, pl, pr)] = 0
    same_bits(X.cpu(), want, "zero_halo")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,S,k,stride,kpad", [(2, 400, 10, 5, 16), (1, 10, 10, 5, 16), (3, 50, 16, 3, 16), (2, 82510, 10, 5, 16)])
def test_unfold_rows(cuda, B, S, k, stride, kpad, dtype):
    """Class A (the last shape: 2 x 16 501 x 16 = 528 032 elements, past one grid)."""
    wav = vals(10)[:B * S].view(B, S)
    L = (S - k) // stride + 1
    W, O = Buf((B, S), FP, cuda, 0, wav), Buf((B * L, kpad), dtype, cuda, 0)
    call("st5_unfold_rows", W.ptr, O.ptr, B, S, k, stride, kpad, hip.dt(dtype), hip.stream())
    sync_intact(O)
    same_bits(O.cpu(), E.unfold_rows(wav, k, stride, kpad).to(dtype), "unfold_rows")


@pytest.mark.parametrize("keep", [1.0, 0.0, -0.0], ids=["keep", "drop", "minus-zero"])
@pytest.mark.parametrize("nbytes", [16, 16 * 257, (8 << 20) + 48])
def test_select_moves_bytes(cuda, nbytes, keep):
    """select, select_bwd, skip_grad on random 32-bit patterns (NaN payloads included): class A.  -0.0 compares equal to zero: dropped."""
    n = nbytes // 4
    g = gen(nbytes)
    a, b, d0 = (torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(I32) for _ in range(3))
    a[:4] = torch.tensor([0x7FC00001, 0x7F800001, -1, 0x7FFFFFFF], dtype=torch.int64).to(I32)       # NaNs with payloads
    K = torch.tensor([keep], device=cuda)
    A_, B_, D0 = Buf(n, I32, cuda, 0, a), Buf(n, I32, cuda, 0, b), Buf(n, I32, cuda, 0, d0)
    Y, GA, GB = Buf(n, I32, cuda, 0), Buf(n, I32, cuda, 0), Buf(n, I32, cuda, 0)
    s = hip.stream()
    call("st5_select", K.data_ptr(), A_.ptr, B_.ptr, Y.ptr, nbytes, s)
    call("st5_select_bwd", K.data_ptr(), A_.ptr, GA.ptr, GB.ptr, nbytes, s)
    call("st5_skip_grad", K.data_ptr(), A_.ptr, D0.ptr, nbytes, s)
    sync_intact(Y, GA, GB, D0)
    kept = keep != 0.0
    zero = torch.zeros(n, dtype=I32)
    assert torch.equal(Y.cpu(), E.select(keep, a, b)), "select"
    assert torch.equal(GA.cpu(), zero if kept else a) and torch.equal(GB.cpu(), a if kept else zero), "select_bwd"
    assert torch.equal(D0.cpu(), d0 if kept else a), "skip_grad"


def test_select_argument_errors(cuda):
    L, s = hip.lib(), hip.stream()
    K = torch.ones(1, device=cuda)
    A_, B_, Y = Buf(16, I32, cuda, 0, "sent"), Buf(16, I32, cuda, 0, "sent"), Buf(16, I32, cuda, 0, "sent")
    U = Buf(16, I32, cuda, 1, "sent")
    assert L.st5_select(K.data_ptr(), A_.ptr, B_.ptr, Y.ptr, 24, s) == ERR_ARG
    assert L.st5_select_bwd(K.data_ptr(), A_.ptr, B_.ptr, Y.ptr, 24, s) == ERR_ARG
    assert L.st5_skip_grad(K.data_ptr(), A_.ptr, Y.ptr, 24, s) == ERR_ARG
    for p in ((U.ptr, B_.ptr, Y.ptr), (A_.ptr, U.ptr, Y.ptr), (A_.ptr, B_.ptr, U.ptr)):
        assert L.st5_select(K.data_ptr(), *p, 32, s) == ERR_ALIGN
        assert L.st5_select_bwd(K.data_ptr(), *p, 32, s) == ERR_ALIGN
    assert L.st5_skip_grad(K.data_ptr(), U.ptr, Y.ptr, 32, s) == ERR_ALIGN and L.st5_skip_grad(K.data_ptr(), A_.ptr, U.ptr, 32, s) == ERR_ALIGN
    sync_intact(A_, B_, Y, U)
    for b in (A_, B_, Y, U):
        assert bool(torch.all(b.t == SENT_I))


# ---- log-mel front end -------------------------------------------------------------------------------------------------------------
def test_stft_frames_and_rows(cuda):
    """Class A: st5_stft_frames at n_fft = 16, hop = 4 against reflect-padded framing (S = 9 is the smallest accepted); the ragged
    form over three items (the minimum included) equals the per-item kernel and the reference."""
    n_fft, hop, s = 16, 4, hip.stream()
    per_item = {}
    for S in (9, 10, 33, 64):
        wav = vals(11)[:2 * S].view(2, S)
        L = 1 + S // hop
        W, O = Buf((2, S), FP, cuda, 0, wav), Buf((2, L, n_fft), FP, cuda, 0)
        call("st5_stft_frames", W.ptr, O.ptr, 2, S, n_fft, hop, s)
        sync_intact(O)
        same_bits(O.cpu(), E.stft_frames(wav, n_fft, hop), f"stft_frames S={S}")
        per_item[S] = (wav[0], O.cpu()[0])
    assert hip.lib().st5_stft_frames(W.ptr, O.ptr, 2, 8, n_fft, hop, s) == ERR_ARG
    lens = [33, 9, 64]
    wavs = [Buf(S, FP, cuda, 0, per_item[S][0]) for S in lens]
    off = [0]
    for S in lens:
        off.append(off[-1] + 1 + S // hop)
    P = torch.tensor([w.ptr for w in wavs], dtype=torch.int64, device=cuda)
    LN = torch.tensor(lens, dtype=I32, device=cuda)
    FO = torch.tensor(off, dtype=torch.int64, device=cuda)
    O = Buf((off[-1], n_fft), FP, cuda, 0)
    call("st5_stft_frames_rows", P.data_ptr(), LN.data_ptr(), FO.data_ptr(), O.ptr, 3, off[-1], n_fft, hop, s)
    sync_intact(O)
    same_bits(O.cpu(), torch.cat([per_item[S][1] for S in lens]), "stft_frames_rows against per-item stft_frames")
    same_bits(O.cpu(), torch.cat([E.stft_frames(per_item[S][0][None], n_fft, hop)[0] for S in lens]), "stft_frames_rows against the reference")


def test_stft_magnitude_and_log10_floor(cuda):
    """stft_magnitude with nbins < ldh: class B with k = 4, pad columns exact zeros.  log10_floor: class C, values below the floor
    and denormals included, on powers spread evenly in the exponent from 1e-12 to 1e2 (a set that lies almost wholly below the floor
    is one value 2000 times over: the emulation's figure is then that of a single rounding, not of the function)."""
    rows, nbins, ldh, s = 37, 9, 12, hip.stream()
    reim = vals(12)[:rows * 2 * ldh].view(rows, 2 * ldh)
    X, M = Buf((rows, 2 * ldh), FP, cuda, 0, reim), Buf((rows, ldh), FP, cuda, 0)
    call("st5_stft_magnitude", X.ptr, M.ptr, rows, nbins, ldh, s)
    sync_intact(M)
    ref = E.stft_magnitude(reim, nbins, ldh)
    assert bool(torch.all(bits(M.cpu()[:, nbins:]) == 0)), "stft_magnitude: pad columns are not exact zeros"
    hold_b("stft_magnitude", M.cpu(), ref, ref.abs(), 4, FP)
    n = 2055 + 64
    pw = 10.0 ** (torch.rand(n, generator=gen(13)) * 14 - 12)         # powers from 1e-12 to 1e2, a seventh of them below the floor
    pw[:8] = torch.tensor([0.0, 1e-45, 1e-39, 1.1e-38, 1e-11, 1e-10, 1.0000001e-10, 1.0])
    X, Y = Buf(n, FP, cuda, 0, pw), Buf(n, FP, cuda, 0)
    call("st5_log10_floor", X.ptr, Y.ptr, n, 1e-10, s)
    sync_intact(Y)
    hold_c("log10_floor", f"n={n}", "y", E.flat_passes(Y.cpu(), E.log10_floor(pw, 1e-10), E.log10_floor(pw, 1e-10, True), n))
    assert bool(torch.all(bits(Y.cpu()[:5]) == bits(Y.cpu()[5:6]))), "log10_floor: values below the floor do not give log10(floor)"
    settle()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 200), (5, 65), (261, 1), (261, 200), (2100, 256)])
def test_channel_affine(cuda, rows, cols, dtype):
    """y = act(x a + b): NONE / ReLU / LeakyReLU class B (k = 1 + the activation's), GELU / tanh class C on rows.  The last shape
    has 537 600 elements: past one grid."""
    g = gen(rows, cols, 5)
    x = R.rnd(torch.randn(rows, cols, generator=g) * 2, dtype)
    a, b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    X, A_, B_ = Buf((rows, cols), dtype, cuda, 0, x), a.to(cuda), b.to(cuda)
    for act in (E.ACT_NONE, E.ACT_RELU, E.ACT_LRELU_01, E.ACT_GELU, E.ACT_TANH):
        Y = Buf((rows, cols), dtype, cuda, 0)
        call("st5_channel_affine", X.ptr, A_.data_ptr(), B_.data_ptr(), Y.ptr, rows, cols, act, hip.dt(dtype), hip.stream())
        sync_intact(Y)
        ref, terms = E.channel_affine(x, a, b, act)
        if act in E.TRANSCENDENTAL:
            hold_c("channel_affine " + E.ACT_NAMES[act], f"{rows}x{cols} {name(dtype)}", "y", R.passes(Y.cpu().float(), ref, E.channel_affine(x, a, b, act, dtype, True)))
        else:
            hold_b(f"channel_affine {E.ACT_NAMES[act]} {rows}x{cols}", Y.cpu(), ref, terms, 1 + E.act_roundings(act), dtype)
    settle()


# ---- cross entropy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [1, 63, 64, 65])
def test_cross_entropy_edges(cuda, V, dtype):
    """ld in {V, V + 5} x eps in {0, 0.1} x rows in {1, 5}, ignored and negative targets included, the atomic and the _rows form.
    dlogits and the row losses: class C (dlogits on rows, columns [V, ld) exact zeros); the atomic sums (onto non-zero cells): class D."""
    d, s = hip.dt(dtype), hip.stream()
    for ld in (V, V + 5):
        for eps in (0.0, 0.1):
            for rows in (1, 5):
                g = gen(V, ld, rows, int(eps * 10))
                logits = R.rnd(torch.randn(rows, V, generator=g) * 3, dtype)
                tgt = torch.randint(0, V, (rows,), generator=g, dtype=I32)
                ignore = 1 if V > 2 else 7777
                tgt[0] = V - 1                                  # (row 0 always counts)
                if rows > 1:
                    tgt[1], tgt[3] = -100, (ignore if V > 2 else -1)
                    tgt[2] = 0 if V > 2 else tgt[2]
                Lg = torch.full((rows, ld), 50.0)               # (what lies in the pad columns must not be read)
                Lg[:, :V] = logits
                LG, TG = Buf((rows, ld), dtype, cuda, 0, Lg), tgt.to(cuda)
                ref = E.cross_entropy(logits, tgt, eps, ignore, 0.5)
                emu = E.cross_entropy(logits, tgt, eps, ignore, 0.5, dtype, True)
                terms, chain = E.cross_entropy_terms(logits, tgt, eps, ignore)
                case = f"V={V} ld={ld} eps={eps} rows={rows} {name(dtype)}"
                # the _rows form
                RL, RN, DL = Buf(rows, FP, cuda, 0), Buf(rows, FP, cuda, 0), Buf((rows, ld), dtype, cuda, 0)
                call("st5_cross_entropy_rows", LG.ptr, TG.data_ptr(), RL.ptr, RN.ptr, DL.ptr, rows, V, ld, eps, ignore, 0.5, d, s)
                sync_intact(RL, RN, DL)
                dl = DL.cpu()
                assert bool(torch.all(bits(dl[:, V:]) == 0)), f"{case}: dlogits pad columns are not exact zeros"
                hold_c("cross_entropy_rows", case, "dlogits", R.passes(dl[:, :V].float(), ref[2], emu[2]))
                hold_c("cross_entropy_rows", case, "row_loss", R.passes(RL.cpu(), ref[0], emu[0]))
                hold_c("cross_entropy_rows", case, "row_nll", R.passes(RN.cpu(), ref[1], emu[1]))
                # the atomic form, onto non-zero sums
                LS, NS, DA = Buf(1, FP, cuda, 0, torch.tensor([2.5])), Buf(1, FP, cuda, 0, torch.tensor([-1.5])), Buf((rows, ld), dtype, cuda, 0)
                call("st5_cross_entropy", LG.ptr, TG.data_ptr(), LS.ptr, NS.ptr, DA.ptr, rows, V, ld, eps, ignore, 0.5, d, s)
                sync_intact(LS, NS, DA)
                same_bits(DA.cpu(), dl, f"{case}: dlogits of the atomic form against the _rows form")
                for nm, got, k, init in (("loss_sum", LS.cpu(), 0, 2.5), ("nll_sum", NS.cpu(), 1, -1.5)):
                    hold_d(f"cross_entropy {nm} {case}", got, ref[k].sum().item() + init, terms.sum().item() + abs(init), chain + rows)
    settle()
