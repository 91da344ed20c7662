"""The live-frame entry points of csrc/batchnorm.hip and csrc/elementwise.hip through the C ABI (st5_batchnorm_act_fwd_live /
_bwd_live, st5_pad_time_live, st5_zero_rows_live): x is [B, Lx, C] and only the first *live rows of every batch element count, *live
one int32 cell in device memory.  B 3, Lx 32, C in {4, 32, 80} and one case at 512; both activations; both output layouts of the mel
post-net (the haloed bf16 operand of the next convolution, the fp32 output with the residual added).

1. live == Lx: every output -- y, the saved statistics, running_mean / running_var / num_batches_tracked, dx, dgamma, dbeta -- is
   byte-equal to the existing entry points', dropout 0.5 included (the mask hashes the physical element index).
2. live in {24, 17, 2, 1}, dropout 0: against the existing entry points run on the contiguous slice x[:, :live].  Both are judged by an
   fp64 restatement written here; the live variant's maximal error may be at most twice the existing kernel's (the only difference is
   the grouping of the fp64 partial sums, which can move an fp32 result by a last bit).  Dead rows of every output are exact zeros,
   halo rows are zeros.  Both errors are printed, and appended to the file ST5_PARITY_OUT names (how
   profiles/t2s_fixed_shape_parity.txt was written).
3. dropout 0.5 on running statistics, live 17: dx != 0 exactly where y != 0 (gamma, dy > 0): the backward regenerates the forward's mask.
4. st5_pad_time_live and st5_zero_rows_live against torch indexing, a cell outside [0, Lx] included (the kernels clamp)."""
import os

import pytest
import torch

from speecht5_amd import hip

pytestmark = pytest.mark.gpu
FP, BF = torch.float32, torch.bfloat16
B, LX, PAD, EPS, MOM = 3, 32, 2, 1e-5, 0.1
SENT = 7.0
CASES = [(C, act, layout) for C in (4, 32, 80) for act in ("tanh", "none") for layout in ("halo", "f32res")] + [(512, "tanh", "halo")]
IDS = [f"C{C}-{act}-{layout}" for C, act, layout in CASES]


def _report(line):
    print(line)
    path = os.environ.get("ST5_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _inputs(C, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * C + seed)
    x = torch.randn(B, LX, C, generator=g) * 1.5 + torch.linspace(-1, 1, C)
    dy = torch.randn(B, LX, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    res = torch.randn(B, LX, C, generator=g).to(BF)
    rm, rv = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
    g0, b0 = torch.full((C,), 0.75), torch.linspace(-1, 1, C)
    return {k: v.to(dev) for k, v in dict(x=x, dy=dy, gamma=gamma, beta=beta, res=res, rm=rm, rv=rv, g0=g0, b0=b0).items()}


def _run(dev, inp, Lx, act, layout, live, training=1, p=0.0, seed=0x5EED):
    """Forward + backward through the plain (live None) or the live entry points on inp["x"][:, :Lx] -> every output, as written."""
    L = hip.lib()
    x, dy, res = (inp[k][:, :Lx].contiguous() for k in ("x", "dy", "res"))
    C, rows = x.shape[2], B * Lx
    RM, RV, NB = inp["rm"].clone(), inp["rv"].clone(), torch.tensor([5], dtype=torch.int64, device=dev)
    ST = torch.full((2 * C,), SENT, device=dev)
    ws = hip.workspace(L.st5_batchnorm_ws_bytes(C), dev)
    halo_map = (Lx, (Lx + 2 * PAD) * C, PAD * C, PAD)
    if layout == "halo":
        Y, omap, yf32, Rp = torch.full((B, Lx + 2 * PAD, C), SENT, dtype=BF, device=dev), halo_map, 0, 0
    else:
        Y, omap, yf32, Rp = torch.full((B, Lx, C), SENT, dtype=FP, device=dev), (0, 0, 0, 0), 1, res.data_ptr()
    a = hip.ACT_TANH if act == "tanh" else hip.ACT_NONE
    head = (x.data_ptr(), inp["gamma"].data_ptr(), inp["beta"].data_ptr(), RM.data_ptr(), RV.data_ptr(), NB.data_ptr(), MOM, EPS, training, a,
            p, seed, Rp, Y.data_ptr(), yf32, ST.data_ptr(), ws.data_ptr(), rows, C, *omap)
    if live is None:
        hip.check(L.st5_batchnorm_act_fwd(*head, hip.dt(BF), hip.stream()), "st5_batchnorm_act_fwd")
    else:
        hip.check(L.st5_batchnorm_act_fwd_live(*head, live.data_ptr(), Lx, hip.dt(BF), hip.stream()), "st5_batchnorm_act_fwd_live")
    DX = torch.full((B, Lx + 2 * PAD, C), SENT, dtype=BF, device=dev)
    DG, DB = inp["g0"].clone(), inp["b0"].clone()
    head = (x.data_ptr(), dy.data_ptr(), ST.data_ptr(), inp["gamma"].data_ptr(), inp["beta"].data_ptr(), DG.data_ptr(), DB.data_ptr(), training,
            a, p, seed, DX.data_ptr(), ws.data_ptr(), rows, C, *halo_map)
    if live is None:
        hip.check(L.st5_batchnorm_act_bwd(*head, hip.dt(BF), hip.stream()), "st5_batchnorm_act_bwd")
    else:
        hip.check(L.st5_batchnorm_act_bwd_live(*head, live.data_ptr(), Lx, hip.dt(BF), hip.stream()), "st5_batchnorm_act_bwd_live")
    torch.cuda.synchronize()
    return {"y": Y, "stats": ST, "running_mean": RM, "running_var": RV, "nbt": NB, "dx": DX, "dgamma": DG, "dbeta": DB}


def _rows(t, layout):
    """(the Lx data rows, the halo rows) of an output buffer."""
    if layout == "halo":
        return t[:, PAD:-PAD], torch.cat([t[:, :PAD], t[:, -PAD:]], 1)
    return t, t[:, :0]


def _fp64(inp, n, act, layout):
    """The post-net block on the slice [:, :n] in fp64 (dropout 0): torch's BatchNorm1d in training mode, tanh, the residual, and the
    gradients of the block WITHOUT the residual, dgamma / dbeta accumulated onto their starting values."""
    x, dy = inp["x"][:, :n].double().cpu(), inp["dy"][:, :n].double().cpu()
    gamma, beta = inp["gamma"].double().cpu(), inp["beta"].double().cpu()
    cnt = B * n
    mean = x.mean((0, 1))
    var = ((x - mean) ** 2).mean((0, 1))
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = (x - mean) * rstd
    z = xh * gamma + beta
    ya = torch.tanh(z) if act == "tanh" else z
    y = ya + inp["res"][:, :n].double().cpu() if layout == "f32res" else ya
    unb = var * cnt / (cnt - 1) if cnt > 1 else var
    g = dy * (1 - ya * ya) if act == "tanh" else dy
    s1, s2 = g.sum((0, 1)), (g * xh).sum((0, 1))
    dx = gamma * rstd * (g - s1 / cnt - xh * s2 / cnt)
    return {"y": y, "mean": mean, "rstd": rstd, "running_mean": (1 - MOM) * inp["rm"].double().cpu() + MOM * mean,
            "running_var": (1 - MOM) * inp["rv"].double().cpu() + MOM * unb, "dx": dx,
            "dgamma": inp["g0"].double().cpu() + s2, "dbeta": inp["b0"].double().cpu() + s1}


def _errors(out, ref, n, layout):
    C = ref["mean"].numel()
    got = {"y": _rows(out["y"], layout)[0][:, :n], "mean": out["stats"][:C], "rstd": out["stats"][C:], "running_mean": out["running_mean"],
           "running_var": out["running_var"], "dx": _rows(out["dx"], "halo")[0][:, :n], "dgamma": out["dgamma"], "dbeta": out["dbeta"]}
    return {k: float((v.double().cpu() - ref[k]).abs().max()) for k, v in got.items()}


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


# ---- 1 ----
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("C,act,layout", CASES, ids=IDS)
def test_all_rows_live_is_the_existing_kernel_bit_for_bit(cuda, C, act, layout, p):
    inp = _inputs(C, cuda)
    live = torch.tensor([LX], dtype=torch.int32, device=cuda)
    for training in (1, 0):
        want = _run(cuda, inp, LX, act, layout, None, training, p if training else 0.0)
        got = _run(cuda, inp, LX, act, layout, live, training, p if training else 0.0)
        for k in want:
            assert _bytes_equal(want[k], got[k]), (k, training)
        assert int(got["nbt"]) == 5 + training
        if p and training:       # the dropout did something: the comparison is not of two unmasked runs
            data = _rows(got["y"], layout)[0]
            assert 0.3 < float((data == (inp["res"].float() if layout == "f32res" else 0)).float().mean()) < 0.7


# ---- 2 ----
@pytest.mark.parametrize("n", [24, 17, 2, 1])
@pytest.mark.parametrize("C,act,layout", CASES, ids=IDS)
def test_live_rows_against_the_existing_kernel_on_the_slice(cuda, C, act, layout, n):
    inp = _inputs(C, cuda, seed=n)
    live = torch.tensor([n], dtype=torch.int32, device=cuda)
    got = _run(cuda, inp, LX, act, layout, live)
    plain = _run(cuda, inp, n, act, layout, None)
    ref = _fp64(inp, n, act, layout)
    e_live, e_plain = _errors(got, ref, n, layout), _errors(plain, ref, n, layout)
    for k in e_live:
        _report(f"batchnorm_live C={C} act={act} layout={layout} live={n} {k}: live kernel {e_live[k]:.3e}  existing kernel on the slice {e_plain[k]:.3e}")
    assert int(got["nbt"]) == int(plain["nbt"]) == 6
    # dead rows and halo rows of both outputs are exact zeros (the buffers were filled with 7.0)
    for name, lay in (("y", layout), ("dx", "halo")):
        data, halo = _rows(got[name], lay)
        assert bool((data[:, n:] == 0).all()) and not bool(torch.signbit(data[:, n:].float()).any()), f"{name}: dead rows"
        assert bool((halo == 0).all()), f"{name}: halo rows"
        assert bool((data[:, :n] != SENT).all()), f"{name}: live rows written"
    for k in e_live:
        assert e_live[k] <= 2 * e_plain[k], (k, e_live[k], e_plain[k])


# ---- 3 ----
@pytest.mark.parametrize("act", ["tanh", "none"])
@pytest.mark.parametrize("C,layout", [(32, "halo"), (80, "f32res")])
def test_backward_regenerates_the_forward_dropout_mask(cuda, C, layout, act):
    n = 17
    inp = _inputs(C, cuda, seed=3)
    inp["dy"] = inp["dy"].abs() + 0.5
    inp["res"] = torch.zeros_like(inp["res"])
    inp["x"] = inp["x"].clamp(-1.5, 1.5)    # (|z| < 6: tanh stays off +-1 in fp32, its derivative is not rounded to zero)
    live = torch.tensor([n], dtype=torch.int32, device=cuda)
    out = _run(cuda, inp, LX, act, layout, live, training=0, p=0.5)
    y, dx = _rows(out["y"], layout)[0], _rows(out["dx"], "halo")[0]
    assert torch.equal(y != 0, dx != 0)
    kept = float((y[:, :n] != 0).float().mean())
    assert 0.4 < kept < 0.6 and not bool((y[:, n:] != 0).any())
    assert _bytes_equal(out["running_mean"], inp["rm"]) and _bytes_equal(out["running_var"], inp["rv"]) and int(out["nbt"]) == 5


# ---- 4 ----
@pytest.mark.parametrize("dtype", [FP, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [32, 24, 17, 2, 1, 0, -3, 40])
def test_pad_time_live_and_zero_rows_live_against_indexing(cuda, n, dtype):
    L = hip.lib()
    c = min(max(n, 0), LX)
    live = torch.tensor([n], dtype=torch.int32, device=cuda)
    for C in (4, 80, 200):
        g = torch.Generator().manual_seed(C)
        src = (torch.randn(B, LX, C, generator=g) + 3.0).to(dtype).to(cuda)
        dst = torch.full((B, LX + 2 * PAD, C), SENT, dtype=dtype, device=cuda)
        hip.check(L.st5_pad_time_live(src.data_ptr(), dst.data_ptr(), B, LX, C, PAD, PAD, live.data_ptr(), hip.dt(dtype), hip.stream()),
                  "st5_pad_time_live")
        want = torch.zeros_like(dst)
        want[:, PAD:PAD + c] = src[:, :c]
        assert _bytes_equal(dst, want), (C, "pad")
        if n == LX:      # nothing dead: st5_pad_time's bytes
            plain = torch.full_like(dst, SENT)
            hip.check(L.st5_pad_time(src.data_ptr(), plain.data_ptr(), B, LX, C, PAD, PAD, hip.dt(dtype), hip.stream()), "st5_pad_time")
            assert _bytes_equal(dst, plain)
        if dtype == FP:
            buf = src.clone()
            hip.check(L.st5_zero_rows_live(buf.data_ptr(), B, LX, C, live.data_ptr(), hip.stream()), "st5_zero_rows_live")
            want = src.clone()
            want[:, c:] = 0
            assert _bytes_equal(buf, want), (C, "zero rows")
