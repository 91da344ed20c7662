"""csrc/norm.hip, csrc/softmax.hip and csrc/batchnorm.hip, through the C ABI, against the fp64 references of tests/norm_reference.py at
the shapes training runs: LayerNorm backward with two, three and more trips of the ping-pong loop (rows > 4096), every vector width
full and partially filled, the scalar kernels, every argument form; all four softmax instantiations with the recipe's 320 buckets; the
BatchNorm partial-sum kernels at their 64-block cap.

Bars (norm_reference.passes).  Per tensor: worst row (column, for the quantities reduced over rows) of
||kernel - fp64|| / max(||fp64 row||, 2^-8 * largest row norm), held to BAR = 4 x the worst row of the emulation on the same case
(the same arithmetic in fp32 with the kernels' rounding points; its own size is capped in tests/test_norm_reference_cpu.py).
dgamma, dbeta and dQP are summed over rows in an order the emulation does not reproduce (per-lane register sums, 4 waves through LDS,
block partials folded 16 at a time; LDS atomics in arrival order).  For them an element also passes inside the deterministic bound
gamma_n * sum |t|, gamma_n = n u / (1 - n u), u = 2^-24: every fp32 sum of the terms t whose longest addition chain has n links lies
within it of the exact sum.  n = a lane's rows (4 per trip) + 4 waves + the partials chain (ceil(blocks / 16) + 16) + 1 for the
accumulation + 1 for the rounding of the term itself (norm_reference.ln_sum_chain); for dQP n = the keys of the fullest bucket; sum |t|
comes from the fp64 reference (plus |initial value| of an accumulated buffer).  BatchNorm's dgamma / dbeta are summed in fp64: what is
left of the chain is the cast of the sum and the accumulation into the fp32 buffer, n = 2 on |sum| + |initial value|.
Nothing in a bar comes from a kernel's output.
A constant row has no condition number (fp64: xhat = 0 exactly): its rows are judged after norm_reference.constant_row_delta's bound
is taken off.  Rows of a fully padded batch item are the only ones left out of a comparison; they must be exact zeros.

Every output carries a sentinel-filled guard region (and, in mapped layouts, sentinel-filled gaps between the batch blocks) that
must come back bit-identical; everything runs under util.poisoned_allocations(); each test makes one pass.  Also beyond the
issue's list: T = 331 at S = 499, because with T <= 160 queries no pair reaches the upper clip bucket (i - j >= 159).
The measured kernel / emulation ratios of an MI355X run are in profiles/norm_fp64_ratios.txt."""
import math

import numpy as np
import pytest
import torch

from oracle.speecht5_oracle import conv_out_lengths
from speecht5_amd import hip
from tests import attention_reference as A
from tests import norm_reference as R
from tests.util import poisoned_allocations

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
DTYPES = [BF, FP]
IDS = ["bf16", "fp32"]
EPS = 1e-5
SENT = -7.25          # exact in bf16
GUARD = 4096
MAXREL = 160
LN_DEFAULT_BLOCKS = 256


def guarded(shape, dtype, dev, init=None):
    """(view, flat): `view` is the output the kernel gets (NaN-filled, or a copy of `init`), followed in memory by GUARD sentinels."""
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), SENT, dtype=dtype, device=dev)
    if init is None:
        flat[:n] = float("nan") if dtype.is_floating_point else -1
    else:
        flat[:n] = init.reshape(-1).to(dtype)
    return flat[:n].view(shape), flat


def guards_intact(*flats):
    for k, f in enumerate(flats):
        assert torch.all(f[-GUARD:].float() == SENT), f"guard region of output {k} overwritten"


def report(family, case, nm, ek, ee):
    print(f"norm fp64 pin: {family} | {case} | {nm} | kernel {ek:.3e} emulation {ee:.3e} ratio {ek / ee if ee > 0 else (0.0 if ek == 0 else math.inf):.3f}")


_missed = []


def hold(family, case, nm, got, ref, emu, **kw):
    """One tensor against its bar; a miss is recorded and raised by settle() once the whole case has been measured and printed
    (every case function empties the list when it starts, so nothing survives a test that ended early)."""
    ok, ek, ee = R.passes(got.cpu(), ref, emu, **kw)
    report(family, case, nm, ek, ee)
    if not ok:
        _missed.append(f"{family} {case} {nm}: kernel worst row {ek:.3e}, emulation {ee:.3e} (bar {R.BAR} x)")


def settle():
    missed = list(_missed)
    _missed.clear()
    assert not missed, "; ".join(missed)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
VEC_WIDTHS = [80, 256, 512, 516, 768, 1024, 1028, 1280, 1536, 2048]
SCALAR_WIDTHS = [30, 767, 2052, 2056, 4096]
ROWS = [1, 15, 16, 17, 3992, 8192, 8200, 16408]     # 16-row block tail; one trip; two; two and three (171 blocks); three and more
_FAMILY_OF_ROWS = {1: "hard", 15: "hard", 16: "edge", 17: "hard", 3992: "edge", 8192: "hard", 8200: "randn", 16408: "edge"}
LN_CASES = sorted({(r, c, _FAMILY_OF_ROWS[r]) for r in ROWS for c in (768, 1024)} |
                  {(17, c, "hard") for c in VEC_WIDTHS + SCALAR_WIDTHS} | {(8200, c, "randn") for c in VEC_WIDTHS + SCALAR_WIDTHS} |
                  {(8200, c, "hard") for c in (516, 1536, 2048, 2052)})


def ln_forward(dev, x, gamma, beta, dtype, gelu=False, keep=None, skip=None):
    L = hip.lib()
    rows, cols = x.shape
    X, G, Bt = x.to(dev), gamma.to(dev), beta.to(dev)
    Y, fy = guarded((rows, cols), dtype, dev)
    M, fm = guarded((rows,), FP, dev)
    Rs, fr = guarded((rows,), FP, dev)
    a = (X.data_ptr(), G.data_ptr(), Bt.data_ptr(), Y.data_ptr(), M.data_ptr(), Rs.data_ptr(), rows, cols, EPS)
    if gelu:
        hip.check(L.st5_layernorm_gelu_fwd(*a, hip.dt(dtype), hip.stream()), "st5_layernorm_gelu_fwd")
    elif keep is not None:
        hip.check(L.st5_layernorm_gated_fwd(*a, keep.data_ptr(), skip.data_ptr(), hip.dt(dtype), hip.stream()), "st5_layernorm_gated_fwd")
    else:
        hip.check(L.st5_layernorm_fwd(*a, hip.dt(dtype), hip.stream()), "st5_layernorm_fwd")
    torch.cuda.synchronize()
    guards_intact(fy, fm, fr)
    return X, G, Bt, Y, M, Rs


def ln_backward(dev, DY, X, G, M, Rs, dtype, g0, b0, form="full", Bt=None, addend=None, drop=None, keep=None):
    """form: full | dgamma | dbeta | neither | nodx.  Returns dx, dgamma, dbeta, dx_dropped (None where not asked for)."""
    L = hip.lib()
    rows, cols = X.shape
    DX, fdx = guarded((rows, cols), dtype, dev) if form != "nodx" else (None, None)
    DG, fg = guarded((cols,), FP, dev, g0) if form in ("full", "dgamma", "nodx") else (None, None)
    DB, fb = guarded((cols,), FP, dev, b0) if form in ("full", "dbeta", "nodx") else (None, None)
    DXD, fd = guarded((rows, cols), dtype, dev) if drop is not None else (None, None)
    ws = hip.workspace(L.st5_layernorm_bwd_ws_bytes(rows, cols), dev)     # (queried after any st5_layernorm_set_max_blocks)
    head = (DY.data_ptr(), X.data_ptr(), G.data_ptr())
    mid = (M.data_ptr(), Rs.data_ptr(), hip.ptr(DX), hip.ptr(DG), hip.ptr(DB), ws.data_ptr(), rows, cols)
    seed, p = drop if drop is not None else (0, 0.0)
    if Bt is not None:
        hip.check(L.st5_layernorm_gelu_bwd(*head, Bt.data_ptr(), *mid, hip.dt(dtype), hip.stream()), "st5_layernorm_gelu_bwd")
    elif addend is not None:
        hip.check(L.st5_layernorm_bwd_add(*head, *mid, addend.data_ptr(), hip.dt(dtype), hip.stream()), "st5_layernorm_bwd_add")
    elif keep is not None:
        hip.check(L.st5_layernorm_gated_bwd(*head, *mid, hip.ptr(DXD), p, seed, keep.data_ptr(), hip.dt(dtype), hip.stream()), "st5_layernorm_gated_bwd")
    else:
        hip.check(L.st5_layernorm_bwd(*head, *mid, hip.ptr(DXD), p, seed, hip.dt(dtype), hip.stream()), "st5_layernorm_bwd")
    torch.cuda.synchronize()
    guards_intact(*[f for f in (fdx, fg, fb, fd) if f is not None])
    return DX, DG, DB, DXD


def ln_case(dev, rows, cols, dtype, family, form="full", max_blocks=LN_DEFAULT_BLOCKS, gelu=False, addend=False, drop=None, tag="layernorm"):
    _missed.clear()
    case = f"{rows}x{cols} {family} {IDS[DTYPES.index(dtype)]} {form} cap={max_blocks}"
    x, gamma, beta, dy = R.ln_inputs(rows, cols, dtype, family)
    gen = torch.Generator().manual_seed(rows + cols)
    g0, b0 = torch.randn(cols, generator=gen), torch.randn(cols, generator=gen)
    add = torch.randn(rows, cols, generator=gen).to(dtype) if addend else None
    with poisoned_allocations():
        X, G, Bt, Y, M, Rs = ln_forward(dev, x, gamma, beta, dtype, gelu=gelu)
        DX, DG, DB, DXD = ln_backward(dev, dy.to(dev), X, G, M, Rs, dtype, g0, b0, form, Bt=Bt if gelu else None,
                                      addend=add.to(dev) if addend else None, drop=drop)
    y, mean, rstd = R.layernorm_fwd(x, gamma, beta, EPS, gelu=gelu)
    ye, me, re = R.layernorm_fwd(x, gamma, beta, EPS, dtype=dtype, emulate=True, gelu=gelu)
    kw = dict(beta=beta if gelu else None, addend=add, drop=drop, dgamma0=g0, dbeta0=b0)
    ref = R.layernorm_bwd(dy, x, gamma, mean, rstd, **kw)
    emu = R.layernorm_bwd(dy, x, gamma, me, re, dtype=dtype, emulate=True, **kw)
    sy = sdx = extra = None
    if family == "edge":      # row 0 is the constant 1.5 (norm_reference.constant_row_delta)
        delta = R.constant_row_delta(1.5, EPS)
        gmax = (dy[0].double() * gamma.double()).abs().max().item()
        sy, sdx = torch.zeros(rows, dtype=torch.float64), torch.zeros(rows, dtype=torch.float64)
        sy[0] = delta * gamma.double().norm().item()
        sdx[0] = 2 * rstd[0].item() * delta * delta * gmax * math.sqrt(cols)
        extra = delta * dy[0].double().abs()
    hold(tag, case, "y", Y, y, ye, slack=sy)
    hold(tag, case, "mean", M, mean, me)
    hold(tag, case, "rstd", Rs, rstd, re)
    if DX is not None:
        hold(tag, case, "dx", DX, ref["dx"], emu["dx"], slack=sdx)
    chain = R.ln_sum_chain(rows, max_blocks)
    if DG is not None:
        hold(tag, case, "dgamma", DG, ref["dgamma"], emu["dgamma"], floor=R.summation_floor(ref["abs_dgamma"] + g0.abs(), chain, extra))
    if DB is not None:
        hold(tag, case, "dbeta", DB, ref["dbeta"], emu["dbeta"], floor=R.summation_floor(ref["abs_dbeta"] + b0.abs(), chain))
    if DXD is not None:       # bit for bit: the restated mask times the ROUNDED dx the kernel itself wrote
        seed, p = drop
        scale = torch.from_numpy(R.keep_mask_rows(seed, p, rows, cols)).float() * np.float32(A.inv_keep(p)).item()
        want = (DX.cpu().float() * scale).to(dtype)
        bits = torch.int16 if dtype == BF else torch.int32
        assert torch.equal(DXD.cpu().view(bits), want.view(bits)), f"{case}: dx_dropped != mask x rounded dx"
        hold(tag, case, "dx_dropped", DXD, ref["dxd"], emu["dxd"])
    settle()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,cols,family", LN_CASES, ids=[f"{r}x{c}-{f}" for r, c, f in LN_CASES])
def test_layernorm_rows_and_widths(cuda, rows, cols, family, dtype):
    ln_case(cuda, rows, cols, dtype, family)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,cols,cap", [(300, 768, 1), (300, 768, 2), (300, 80, 3), (100, 1024, 2), (250, 1536, 3), (330, 516, 1)])
def test_layernorm_backward_capped_blocks_every_exit_branch(cuda, rows, cols, cap, dtype):
    """st5_layernorm_set_max_blocks(1, 2, 3): every wave makes 3 ... 20 trips and leaves the ping-pong loop through either break
    (odd / even trip counts, waves with one trip fewer than their neighbours)."""
    L = hip.lib()
    lo, hi = R.ln_trips(rows, cap)
    assert hi >= 3
    hip.check(L.st5_layernorm_set_max_blocks(cap), "st5_layernorm_set_max_blocks")
    try:
        assert L.st5_layernorm_bwd_ws_bytes(rows, cols) >= R.ln_blocks(rows, cap) * 2 * cols * 4
        ln_case(cuda, rows, cols, dtype, "hard", max_blocks=cap)
    finally:
        hip.check(L.st5_layernorm_set_max_blocks(LN_DEFAULT_BLOCKS), "st5_layernorm_set_max_blocks")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", ["dgamma", "dbeta", "neither", "nodx"])
@pytest.mark.parametrize("rows,cols", [(8200, 768), (17, 1028), (8200, 2052)])
def test_layernorm_backward_argument_forms(cuda, rows, cols, form, dtype):
    """dgamma only, dbeta only, neither (the PG = false instantiation), dx == NULL (the column-reduction path)."""
    ln_case(cuda, rows, cols, dtype, "randn", form=form)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["addend", "drop0.1", "drop0.5"])
def test_layernorm_backward_variants_at_text_microbatch(cuda, variant, dtype):
    """8192 x 768, the text micro-batch of the benched update (two trips): st5_layernorm_bwd_add and the dropped second output."""
    drop = (0x51ED + int(10 * float(variant[4:])), float(variant[4:])) if variant.startswith("drop") else None
    ln_case(cuda, 8192, 768, dtype, "randn", addend=variant == "addend", drop=drop)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("keep", [0.0, 1.0])
def test_layernorm_layerdrop_gate_at_text_microbatch(cuda, keep, dtype):
    rows, cols = 8192, 768
    _missed.clear()
    case = f"{rows}x{cols} gate keep={keep} {IDS[DTYPES.index(dtype)]}"
    x, gamma, beta, dy = R.ln_inputs(rows, cols, dtype, "randn", seed=9)
    gen = torch.Generator().manual_seed(5)
    g0, b0, skip = torch.randn(cols, generator=gen), torch.randn(cols, generator=gen), torch.randn(rows, cols, generator=gen).to(dtype)
    K = torch.tensor([keep], device=cuda)
    with poisoned_allocations():
        X, G, Bt, Y, M, Rs = ln_forward(cuda, x, gamma, beta, dtype, keep=K, skip=skip.to(cuda))
        DX, DG, DB, DXD = ln_backward(cuda, dy.to(cuda), X, G, M, Rs, dtype, g0, b0, drop=(77, 0.1), keep=K)
    y, mean, rstd = R.layernorm_fwd(x, gamma, beta, EPS, keep=keep, skip=skip)
    ye, me, re = R.layernorm_fwd(x, gamma, beta, EPS, dtype=dtype, emulate=True, keep=keep, skip=skip)
    hold("layernorm gate", case, "mean", M, mean, me)
    hold("layernorm gate", case, "rstd", Rs, rstd, re)
    if keep == 0:
        assert torch.equal(Y.cpu(), skip) and torch.all(DX == 0) and torch.all(DXD == 0)
        assert torch.equal(DG.cpu(), g0) and torch.equal(DB.cpu(), b0)
        settle()
        return
    ref = R.layernorm_bwd(dy, x, gamma, mean, rstd, keep=keep, dgamma0=g0, dbeta0=b0, drop=(77, 0.1))
    emu = R.layernorm_bwd(dy, x, gamma, me, re, dtype=dtype, emulate=True, keep=keep, dgamma0=g0, dbeta0=b0, drop=(77, 0.1))
    chain = R.ln_sum_chain(rows)
    hold("layernorm gate", case, "y", Y, y, ye)
    hold("layernorm gate", case, "dx", DX, ref["dx"], emu["dx"])
    hold("layernorm gate", case, "dx_dropped", DXD, ref["dxd"], emu["dxd"])
    hold("layernorm gate", case, "dgamma", DG, ref["dgamma"], emu["dgamma"], floor=R.summation_floor(ref["abs_dgamma"] + g0.abs(), chain))
    hold("layernorm gate", case, "dbeta", DB, ref["dbeta"], emu["dbeta"], floor=R.summation_floor(ref["abs_dbeta"] + b0.abs(), chain))
    settle()


EXTRACTOR = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cols", [512, 256])
def test_layernorm_gelu_pair_at_extractor_rows(cuda, cols, dtype):
    """st5_layernorm_gelu_fwd / _bwd at the rows of the layer-norm convolution extractor's layer 5 (the sixth convolution, the first
    with kernel 2) for a 32 x 10 s batch: 32 x 999 = 31 968 rows, 8 trips of the backward loop."""
    rows = 32 * int(conv_out_lengths(torch.tensor([160000]), EXTRACTOR[:6])[0])
    assert rows == 31968 and R.ln_trips(rows)[0] >= 2
    ln_case(cuda, rows, cols, dtype, "randn", gelu=True, tag="layernorm gelu")


def test_layernorm_deferred_reduction_at_multi_trip_rows(cuda):
    """st5_layernorm_defer(1): LayerNorms of widths 80, 768 and 1024 at 8200 rows queued and folded by one flush, more than 48 pending
    (automatic flush), the same dgamma queued twice (flush in between) -- each bit for bit the immediate form."""
    L = hip.lib()
    dev = cuda
    jobs = [(8200, 80), (8200, 768), (8200, 1024)] + [(300, 80)] * 50
    data = []
    for k, (rows, cols) in enumerate(jobs):
        x, gamma, beta, dy = R.ln_inputs(rows, cols, BF, "randn", seed=k)
        X, G, Bt, Y, M, Rs = ln_forward(dev, x, gamma, beta, BF)
        data.append((X, G, M, Rs, dy.to(dev)))
    shared = torch.randn(80, generator=torch.Generator().manual_seed(1))

    def run(deferred):
        outs, flats = [], []
        for k, (rows, cols) in enumerate(jobs):
            if k >= len(jobs) - 2:       # the last two accumulate into ONE pair of buffers
                if k == len(jobs) - 2:
                    pair = guarded((80,), FP, dev, shared), guarded((80,), FP, dev, -shared)
                (DG, fg), (DB, fb) = pair
            else:
                (DG, fg), (DB, fb) = guarded((cols,), FP, dev, torch.full((cols,), 0.5)), guarded((cols,), FP, dev, torch.full((cols,), -0.25))
            X, G, M, Rs, DY = data[k]
            DX, fdx = guarded((rows, cols), BF, dev)
            ws = hip.workspace(L.st5_layernorm_bwd_ws_bytes(rows, cols), dev)
            hip.check(L.st5_layernorm_bwd(DY.data_ptr(), X.data_ptr(), G.data_ptr(), M.data_ptr(), Rs.data_ptr(), DX.data_ptr(), DG.data_ptr(),
                                          DB.data_ptr(), ws.data_ptr(), rows, cols, None, 0.0, 0, hip.BF16, hip.stream()), "st5_layernorm_bwd")
            outs.append((DX, DG, DB))
            flats += [fdx, fg, fb]
        if deferred:
            hip.check(L.st5_layernorm_flush(hip.stream()), "st5_layernorm_flush")
        torch.cuda.synchronize()
        guards_intact(*flats)
        return outs

    with poisoned_allocations():
        immediate = run(False)
        hip.check(L.st5_layernorm_defer(1, hip.stream()), "st5_layernorm_defer")
        try:
            deferred = run(True)
        finally:
            hip.check(L.st5_layernorm_defer(0, hip.stream()), "st5_layernorm_defer")
    for k, (a, b) in enumerate(zip(immediate, deferred)):
        for nm, u, v in zip(("dx", "dgamma", "dbeta"), a, b):
            assert torch.isfinite(u.float()).all() and torch.equal(u, v), f"deferred != immediate: job {k} {jobs[k]} {nm}"


# ---- softmax -----------------------------------------------------------------------------------------------------------------------
S_LDS = [(8, 8), (499, 504), (512, 512), (513, 520), (999, 1000), (1024, 1024), (1500, 1504), (2048, 2048), (2049, 2056), (4093, 4096)]
BH, H = 6, 3


def softmax_case(dev, dtype, T, S, lds, rel=True, causal=False, lens="tail", p=0.0, scale=1.0, extra=True, seed=0xC0FFEE):
    L = hip.lib()
    _missed.clear()
    if lens == "tail":
        lens = [S, max(S - max(S // 5, 1), 1)]
    elif lens == "item_padded":
        lens = [S, 0]
    case = f"T={T} S={S} lds={lds} {IDS[DTYPES.index(dtype)]} rel={int(rel)} causal={int(causal)} lens={lens} p={p} scale={scale}"
    scores, qp, kpm, dP, ex = R.softmax_inputs(BH, H, T, S, lds, MAXREL, dtype, scale=scale, rel=rel, lens=lens)
    ex = ex if extra else None
    nb = 2 * MAXREL if rel else 0
    SC, DPin = scores.clone(), dP.clone()
    SC[..., S:] = float("nan")           # the padding columns S .. lds are never to be read as values
    DPin[..., S:] = float("nan")
    SC = SC.to(dev)
    QP = qp.to(dev) if rel else None
    KP = kpm.to(dev) if kpm is not None else None
    EX = ex.to(dev) if extra else None
    P, fp_ = guarded((BH, T, lds), dtype, dev)
    PD, fpd = guarded((BH, T, lds), dtype, dev) if p > 0 else (None, None)
    DS, fds = guarded((BH, T, lds), dtype, dev, DPin)
    DQ, fdq = guarded((BH, T, nb), dtype, dev) if rel else (None, None)
    with poisoned_allocations():
        hip.check(L.st5_softmax_fwd(SC.data_ptr(), hip.ptr(QP), hip.ptr(KP), P.data_ptr(), hip.ptr(PD), BH, H, T, S, lds, nb, MAXREL if rel else 0,
                                    int(causal), p, seed, hip.dt(dtype), hip.stream()), "st5_softmax_fwd")
        hip.check(L.st5_softmax_bwd(DS.data_ptr(), P.data_ptr(), hip.ptr(EX), hip.ptr(DQ), BH, T, S, lds, nb, MAXREL if rel else 0, p, seed,
                                    hip.dt(dtype), hip.stream()), "st5_softmax_bwd")
    torch.cuda.synchronize()
    guards_intact(*[f for f in (fp_, fpd, fds, fdq) if f is not None])
    a = (scores, qp, kpm, dP, ex, BH, H, T, S, lds, MAXREL if rel else 0, causal, p, seed)
    ref, emu = R.softmax_fwd_bwd(*a), R.softmax_fwd_bwd(*a, dtype=dtype, emulate=True)
    live = ref["live"]
    assert torch.equal(live, emu["live"])
    if lens is not None and lens[1] == 0:
        assert not live[BH // 2:].any() and live[:BH // 2].all()      # one of two items, nothing else, is left out
    else:
        assert live.all()
    got = dict(P=P.cpu(), PD=PD.cpu() if PD is not None else None, dS=DS.cpu(), dQP=DQ.cpu() if rel else None)
    for nm in ("P", "PD", "dS", "dQP"):
        if got[nm] is None:
            continue
        g = got[nm]
        assert torch.all(g[~live] == 0), f"{case} {nm}: rows without a visible key are not exact zeros"
        if nm != "dQP":
            assert torch.all(g[..., S:] == 0), f"{case} {nm}: padding columns S .. lds are not exact zeros"
        floor = None
        if nm == "dQP":
            fullest = int(torch.bincount(R.bucket_table(T, S, MAXREL).reshape(-1)).max())
            floor = R.summation_floor(ref["abs_dQP"], fullest).norm(dim=-1)
        hold("softmax", case, nm, g, ref[nm], emu[nm], select=live, floor=floor)
    if p > 0:
        keep = R.keep_mask_softmax(seed, p, BH * T, S, lds).reshape(BH, T, S)
        assert R.dropout_pattern_ok(got["PD"], got["P"], keep, p, S), f"{case}: dropout pattern / scaling"
    settle()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("S,lds", S_LDS)
def test_softmax_every_instantiation_recipe_buckets(cuda, S, lds, dtype):
    """T = 70 (row count not a multiple of 4), 320 buckets, padding tail, dropout 0.1, dP_extra: NCH = 1, 2, 4, 8 forward and backward."""
    softmax_case(cuda, dtype, 70, S, lds, p=0.1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T", [1, 3, 5])
@pytest.mark.parametrize("S,lds", [(8, 8), (999, 1000), (2049, 2056), (4093, 4096)])
def test_softmax_few_query_rows(cuda, T, S, lds, dtype):
    softmax_case(cuda, dtype, T, S, lds, p=0.3 if T == 3 else 0.0, extra=T != 5)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T,S,lds", [(8, 8, 8), (499, 499, 504), (70, 499, 504), (70, 999, 1000), (5, 1500, 1504), (70, 4093, 4096)])
def test_softmax_causal_with_and_without_offset(cuda, T, S, lds, dtype):
    """S == Tq (training) and S > Tq (incremental: query i sees keys j <= i + S - Tq)."""
    softmax_case(cuda, dtype, T, S, lds, rel=False, causal=True, lens=None, p=0.1, extra=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_softmax_upper_clip_bucket(cuda, dtype):
    """T = 331 > maxrel: pairs with i - j >= 159 fall into the last bucket (with T <= 160 only the lower clip end is ever hit)."""
    softmax_case(cuda, dtype, 331, 499, 504, p=0.1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("S,lds", [(499, 504), (999, 1000), (4093, 4096)])
def test_softmax_fully_padded_item(cuda, S, lds, dtype):
    softmax_case(cuda, dtype, 70, S, lds, lens="item_padded", p=0.1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("S,lds", [(513, 520), (999, 1000), (2048, 2048)])
def test_softmax_scores_of_large_magnitude(cuda, S, lds, dtype):
    softmax_case(cuda, dtype, 70, S, lds, scale=80.0, p=0.3)


# ---- BatchNorm + activation --------------------------------------------------------------------------------------------------------
BN_L, BN_PAD, BN_GAP = 600, 2, 24


def bn_case(dev, rows, C, dtype, training, tanh, p, residual, y_f32, mapped, seed=0xB0B):
    L = hip.lib()
    _missed.clear()
    case = f"{rows}x{C} {IDS[DTYPES.index(dtype)]} train={int(training)} tanh={int(tanh)} p={p} res={int(residual)} yf32={int(y_f32)} map={int(mapped)}"
    x, dy, gamma, beta, res, rmean, rvar = R.bn_inputs(rows, C)
    res = res.to(dtype) if residual else None
    odt = FP if y_f32 else dtype
    g0, b0 = torch.full((C,), 0.75), torch.linspace(-1, 1, C)
    nbatch = rows // BN_L if mapped else 1
    bstride = (BN_L + 2 * BN_PAD) * C + BN_GAP
    omap = (BN_L, bstride, BN_PAD * C, BN_PAD) if mapped else (0, 0, 0, 0)
    X, DYd, G, Bt = x.to(dev), dy.to(dev), gamma.to(dev), beta.to(dev)
    Rd = res.to(dev) if residual else None
    RM, frm = guarded((C,), FP, dev, rmean)
    RV, frv = guarded((C,), FP, dev, rvar)
    NB = torch.tensor([5], dtype=torch.int64, device=dev)
    ST, fst = guarded((2 * C,), FP, dev)
    nout = nbatch * bstride if mapped else rows * C
    act = hip.ACT_TANH if tanh else hip.ACT_NONE
    ws = hip.workspace(L.st5_batchnorm_ws_bytes(C), dev)
    ref_rm, ref_rv, emu_rm, emu_rv, nbt = rmean, rvar, rmean, rvar, 5
    for call in (1, 2):      # the running statistics and the counter after one call and after two
        Y, fy = guarded((nout,), odt, dev, torch.full((nout,), SENT) if mapped else None)
        with poisoned_allocations():
            hip.check(L.st5_batchnorm_act_fwd(X.data_ptr(), G.data_ptr(), Bt.data_ptr(), RM.data_ptr(), RV.data_ptr(), NB.data_ptr(), 0.1, EPS,
                                              int(training), act, p, seed, hip.ptr(Rd), Y.data_ptr(), int(y_f32), ST.data_ptr(), ws.data_ptr(),
                                              rows, C, *omap, hip.dt(dtype), hip.stream()), "st5_batchnorm_act_fwd")
        torch.cuda.synchronize()
        guards_intact(fy, frm, frv, fst)
        a = (0.1, EPS, training, tanh, p, seed)
        ref = R.batchnorm_fwd(x, gamma, beta, ref_rm, ref_rv, nbt, *a, residual=res)
        emu = R.batchnorm_fwd(x, gamma, beta, emu_rm, emu_rv, nbt, *a, residual=res, y_f32=y_f32, dtype=dtype, emulate=True)
        ref_rm, ref_rv, emu_rm, emu_rv, nbt = ref["running_mean"], ref["running_var"], emu["running_mean"], emu["running_var"], ref["nbt"]
        assert int(NB.item()) == nbt == 5 + (call if training else 0), f"{case}: batch counter after call {call}"
        hold("batchnorm", case, f"running_mean call {call}", RM, ref_rm, emu_rm)
        hold("batchnorm", case, f"running_var call {call}", RV, ref_rv, emu_rv)
    Yc = Y.cpu()
    if mapped:
        assert R.mapped_layout_ok(Yc, nbatch, C, BN_L, BN_PAD, bstride, SENT), f"{case}: halo / gaps of y"
        Yc = R.extract_rows(Yc, nbatch, C, BN_L, BN_PAD, bstride)
    hold("batchnorm", case, "y", Yc.reshape(rows, C), ref["y"], emu["y"])
    hold("batchnorm", case, "mean", ST[:C], ref["mean"], emu["mean"])
    hold("batchnorm", case, "rstd", ST[C:], ref["rstd"], emu["rstd"])
    # backward, accumulating into non-zero dgamma / dbeta
    DX, fdx = guarded((nout,), dtype, dev, torch.full((nout,), SENT) if mapped else None)
    DG, fdg = guarded((C,), FP, dev, g0)
    DB, fdb = guarded((C,), FP, dev, b0)
    with poisoned_allocations():
        hip.check(L.st5_batchnorm_act_bwd(X.data_ptr(), DYd.data_ptr(), ST.data_ptr(), G.data_ptr(), Bt.data_ptr(), DG.data_ptr(), DB.data_ptr(),
                                          int(training), act, p, seed, DX.data_ptr(), ws.data_ptr(), rows, C, *omap, hip.dt(dtype), hip.stream()),
                  "st5_batchnorm_act_bwd")
    torch.cuda.synchronize()
    guards_intact(fdx, fdg, fdb)
    rb = R.batchnorm_bwd(x, dy, ref["mean"], ref["rstd"], gamma, beta, training, tanh, p, seed, dgamma0=g0, dbeta0=b0)
    eb = R.batchnorm_bwd(x, dy, emu["mean"], emu["rstd"], gamma, beta, training, tanh, p, seed, dtype=dtype, emulate=True, dgamma0=g0, dbeta0=b0)
    DXc = DX.cpu()
    if mapped:
        assert R.mapped_layout_ok(DXc, nbatch, C, BN_L, BN_PAD, bstride, SENT), f"{case}: halo / gaps of dx"
        DXc = R.extract_rows(DXc, nbatch, C, BN_L, BN_PAD, bstride)
    hold("batchnorm", case, "dx", DXc.reshape(rows, C), rb["dx"], eb["dx"])
    hold("batchnorm", case, "dgamma", DG, rb["dgamma"], eb["dgamma"], floor=R.summation_floor((rb["dgamma"] - g0.double()).abs() + g0.abs(), 1))
    hold("batchnorm", case, "dbeta", DB, rb["dbeta"], eb["dbeta"], floor=R.summation_floor((rb["dbeta"] - b0.double()).abs() + b0.abs(), 1))
    settle()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows", [2, 111, 4097, 19200])
@pytest.mark.parametrize("C", [4, 80, 256, 512, 516, 1024])
def test_batchnorm_tanh_dropout_training(cuda, C, rows, dtype):
    """The post-net's inner blocks: tanh, dropout 0.5, typed output -- in the haloed layout (L = 600, pad = 2) at 19 200 = 32 x 600 rows,
    where C = 256 is cfg 3 at the 64-block cap."""
    bn_case(cuda, rows, C, dtype, True, True, 0.5, False, False, rows == 19200)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tanh,p", [(True, 0.0), (False, 0.0), (False, 0.5)], ids=["tanh-p0", "none-p0", "none-p0.5"])
@pytest.mark.parametrize("rows,C", [(111, 80), (4097, 4), (19200, 256), (19200, 516)])
def test_batchnorm_training_without_dropout_or_activation_typed_output(cuda, rows, C, tanh, p, dtype):
    """Training statistics with p = 0 and with no activation, typed output, haloed at 19 200 rows."""
    bn_case(cuda, rows, C, dtype, True, tanh, p, False, False, rows == 19200)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("rows,C", [(111, 80), (4097, 516), (19200, 80), (19200, 256)])
def test_batchnorm_last_block_fp32_output_with_residual(cuda, rows, C, training, dtype):
    """The post-net's last block: no activation, residual added, fp32 output (`after = before + postnet(before)`)."""
    bn_case(cuda, rows, C, dtype, training, False, 0.5 if training else 0.0, True, True, False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tanh", [True, False], ids=["tanh", "none"])
@pytest.mark.parametrize("rows,C", [(2, 4), (4097, 1024), (19200, 256), (19200, 4)])
def test_batchnorm_eval_statistics_forward_and_backward(cuda, rows, C, tanh, dtype):
    bn_case(cuda, rows, C, dtype, False, tanh, 0.0, False, False, rows == 19200)
