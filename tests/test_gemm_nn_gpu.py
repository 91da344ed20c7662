"""B k-major ("NN") forms of the bf16 LDS-DMA NT kernels: C = epilogue(A . B) with B [K x N] row-major, the data
gradient dX = G . W on the weight as the forward reads it.  Only the B tile's staging and fragment reads differ from the NT kernels, the
MFMA chain is the same, so every check is bit for bit:

* the NN call equals the NT call on an explicitly transposed copy of B, on the same tile kernel (st5_gemm_set_nt_tile, and for the
  128 x 128 kernel every ring depth the dispatch uses);
* the NN call equals the same call under st5_gemm_set_glds(0), the register-staged general kernel;
* for every M, N, K below (partial row / column tiles, 2, 3, 5 and 7 k-tiles: every ring wraps, the phased kernel sees an odd count),
  B as a whole matrix and as a column slice with ld > N, and the epilogues the data gradients use;
* through LinearFunction / FFNFunction with the bf16 mirror active: no transposed copy is registered, same gradients as ST5_DGRAD_NN=0."""
import math
from types import SimpleNamespace

import pytest
import torch

from speecht5_amd import functional as Fn
from speecht5_amd import hip

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
MS, NS, KS = (1, 63, 128, 200, 257), (8, 72, 128, 136, 264), (128, 192, 320, 448)
SLICE_PAD, SLICE_OFF = 24, 8        # B as columns 8 .. 8 + N of a [K, N + 24] matrix: ld > N, 16-byte aligned base
KINDS = ["plain", "bias", "res", "dact", "beta", "drop_res"]

# tile kernel -> (st5_gemm_set_nt_tile, st5_gemm_set_deep_ring, st5_gemm_set_nt_slots).  At these sizes every grid is "at most 256 blocks":
# the 128 x 128 kernel runs its 4- or 3-stage ring from 4 k-tiles on (below: the five-slot ring) unless the deep ring is off; with it off
# and st5_gemm_set_nt_slots(4), two whole stages.
TILES = {"128-ring4": (1, (256, 4), 5), "128-ring3": (1, (256, 3), 5), "128-slots5": (1, (0, 2), 5), "128-ring2": (1, (0, 2), 4),
         "m64": (5, (256, 4), 5), "phased": (3, (256, 4), 5)}


class _knobs:
    """The library's launch choices forced for the block; its defaults afterwards."""

    def __init__(self, tile=0, deep=(256, 4), slots=5, glds=1):
        self.v = (tile, deep, slots, glds)

    @staticmethod
    def _set(tile, deep, slots, glds):
        L = hip.lib()
        hip.check(L.st5_gemm_set_nt_tile(tile), "st5_gemm_set_nt_tile")
        hip.check(L.st5_gemm_set_deep_ring(*deep), "st5_gemm_set_deep_ring")
        hip.check(L.st5_gemm_set_nt_slots(slots), "st5_gemm_set_nt_slots")
        hip.check(L.st5_gemm_set_glds(glds), "st5_gemm_set_glds")

    def __enter__(self):
        self._set(*self.v)

    def __exit__(self, *exc):
        self._set(0, (256, 4), 5, 1)


_INPUTS, _GENERAL = {}, {}


def _inputs(cuda, M, N, K):
    """Operands of one shape, made once and only read afterwards.  B in three forms with the same values: whole [K, N], a column slice
    of a wider matrix, and the transposed copy [N, K] the NT kernels read."""
    key = (M, N, K)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(5 * M + 3 * N + K)
        B = (torch.randn(K, N, generator=g) / math.sqrt(K)).to(BF).to(cuda)
        wide = torch.full((K, N + SLICE_PAD), NAN, dtype=BF, device=cuda)     # (a read outside the slice poisons the result)
        wide[:, SLICE_OFF:SLICE_OFF + N] = B
        _INPUTS[key] = dict(A=(torch.randn(M, K, generator=g) * 0.5).to(BF).to(cuda), B=B, wide=wide, Bt=B.t().contiguous(),
                            bias=torch.randn(N, generator=g).to(cuda), R=torch.randn(M, N, generator=g).to(BF).to(cuda),
                            P=torch.randn(M, N, generator=g).to(BF).to(cuda), C0=torch.randn(M, N, generator=g).to(BF).to(cuda))
    return _INPUTS[key]


def _epilogue(t, N, kind):
    if kind == "plain":
        return dict()
    if kind == "bias":
        return dict(bias=t["bias"])
    if kind == "res":              # F_RES: data gradient plus the relayed residual gradient
        return dict(R=hip.operand(t["R"], N))
    if kind == "dact":             # F_DACT: data gradient through the GELU
        return dict(P=hip.operand(t["P"], N), act=hip.ACT_GELU, flags=hip.DACT, alpha=0.5)
    if kind == "beta":             # F_BETA: accumulate onto the old C
        return dict(beta=1.0)
    if kind == "drop_res":         # F_DROP | F_RES, fixed seed
        return dict(bias=t["bias"], dropout_p=0.1, seed=77, R=hip.operand(t["R"], N))
    raise AssertionError(kind)


def _run(cuda, M, N, K, kind, form):
    """form: 'nn' (B whole), 'nn_slice' (B a column slice), 'nt' (the transposed copy).  No synchronisation: the caller compares on the device."""
    t = _inputs(cuda, M, N, K)
    C = t["C0"].clone() if kind == "beta" else torch.full((M, N), NAN, dtype=BF, device=cuda)
    kw = _epilogue(t, N, kind)
    if form == "nt":
        Bop = hip.operand(t["Bt"], K)
    else:
        kw["flags"] = kw.get("flags", 0) | hip.B_KSTRIDED
        Bop = hip.operand(t["B"], N) if form == "nn" else hip.operand(t["wide"], N + SLICE_PAD, off=SLICE_OFF)
    hip.gemm(hip.operand(t["A"], K), Bop, hip.operand(C, N), M, N, K, hip.BF16, **kw)
    return C


def _general(cuda, M, N, K, kind):
    """The NN call on the general kernel: computed once per (shape, epilogue), shared by every tile kernel's test."""
    key = (M, N, K, kind)
    if key not in _GENERAL:
        with _knobs(glds=0):
            _GENERAL[key] = _run(cuda, M, N, K, kind, "nn")
    return _GENERAL[key]


def _diff(a, b):
    """Number of differing 16-bit patterns, as a device scalar."""
    return (a.view(torch.int16) != b.view(torch.int16)).sum()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tile", list(TILES))
def test_nn_equals_nt_on_the_transposed_copy_and_the_general_kernel(cuda, tile, kind):
    mode, deep, slots = TILES[tile]
    names, bad, nans = [], [], []
    for M in MS:
        for N in NS:
            for K in KS:
                ref = _general(cuda, M, N, K, kind)
                with _knobs(mode, deep, slots):
                    nt = _run(cuda, M, N, K, kind, "nt")
                    whole = _run(cuda, M, N, K, kind, "nn")
                    sliced = _run(cuda, M, N, K, kind, "nn_slice")
                names.append((M, N, K))
                bad.append(torch.stack([_diff(whole, nt), _diff(sliced, nt), _diff(whole, ref)]))
                nans.append(torch.isnan(nt).sum() + torch.isnan(ref).sum())
    bad, nans = torch.stack(bad).cpu(), torch.stack(nans).cpu()
    assert int(nans.sum()) == 0, "NaN in a reference result"
    wrong = [f"{names[i]}: vs NT {int(bad[i, 0])}, slice vs NT {int(bad[i, 1])}, vs general {int(bad[i, 2])}" for i in range(len(names)) if int(bad[i].sum())]
    assert not wrong, f"{tile} {kind}: differing elements -- " + "; ".join(wrong[:8])


@pytest.mark.parametrize("tile", list(TILES))
def test_side_operands_change_the_result(cuda, tile):
    """(the comparisons above would pass if the epilogue ignored its side operands)"""
    mode, deep, slots = TILES[tile]
    with _knobs(mode, deep, slots):
        outs = {k: _run(cuda, 200, 136, 192, k, "nn") for k in KINDS}
    torch.cuda.synchronize()
    for k in KINDS[1:]:
        assert not torch.equal(outs[k], outs["plain"]), k


@pytest.mark.parametrize("tile", list(TILES))
def test_row_split_output(cuda, tile):
    """C (and R) in blocks of 50 rows with two halo rows between them (rpb != 0), the convolution data gradients' layout; M = 200 ends
    blocks inside wave tiles."""
    M, N, K, rpb = 200, 136, 320, 50
    t = _inputs(cuda, M, N, K)
    bs = (rpb + 2) * N
    Rs = torch.randn(M // rpb, rpb + 2, N, generator=torch.Generator().manual_seed(3)).to(BF).to(cuda)
    mode, deep, slots = TILES[tile]

    def run(form, glds=1, m=mode):
        C = torch.full((M // rpb, rpb + 2, N), NAN, dtype=BF, device=cuda)
        kw = dict(R=hip.operand(Rs, N, rpb=rpb, bstride=bs))
        with _knobs(m, deep, slots, glds):
            if form == "nt":
                hip.gemm(hip.operand(t["A"], K), hip.operand(t["Bt"], K), hip.operand(C, N, rpb=rpb, bstride=bs), M, N, K, hip.BF16, **kw)
            else:
                hip.gemm(hip.operand(t["A"], K), hip.operand(t["B"], N), hip.operand(C, N, rpb=rpb, bstride=bs), M, N, K, hip.BF16, flags=hip.B_KSTRIDED, **kw)
        return C
    nn, nt, gen = run("nn"), run("nt"), run("nn", glds=0, m=0)
    torch.cuda.synchronize()
    assert torch.isnan(nn[:, rpb:]).all() and not torch.isnan(nn[:, :rpb]).any(), "halo rows written or block rows missed"
    assert int(_diff(nn[:, :rpb].contiguous(), nt[:, :rpb].contiguous())) == 0
    assert int(_diff(nn[:, :rpb].contiguous(), gen[:, :rpb].contiguous())) == 0


@pytest.mark.parametrize("tile", list(TILES))
def test_dropped_layer_gate_leaves_the_output(cuda, tile):
    mode, deep, slots = TILES[tile]
    keep0, keep1 = torch.zeros(1, device=cuda), torch.ones(1, device=cuda)
    outs = []
    for gate in (keep0, keep1, None):
        prev = hip.set_gate(gate.data_ptr() if gate is not None else 0)
        try:
            with _knobs(mode, deep, slots):
                outs.append(_run(cuda, 257, 264, 448, "res", "nn"))
        finally:
            hip.set_gate(prev)
    torch.cuda.synchronize()
    assert torch.isnan(outs[0]).all(), "a launch under a gate at 0 wrote its output"
    assert not torch.isnan(outs[1]).any() and int(_diff(outs[1], outs[2])) == 0


# ------------------------------------------------------------------------------------------------- the mirror path
def _mirror_backward(cuda, nn_on, monkeypatch):
    """One Linear (stacked pair) + FFN backward in bf16 with the parameters resident in a bf16 mirror; returns (gradients, mirror)."""
    g = torch.Generator().manual_seed(11)
    d, Fd, T = 128, 256, 72
    shapes = dict(wa=(64, d), wb=(64, d), ba=(64,), bb=(64,), w1=(Fd, d), b1=(Fd,), w2=(d, Fd), b2=(d,))
    params, offsets, off = {}, [], 0
    for name, shp in shapes.items():
        scale = 1.0 / math.sqrt(shp[-1]) if len(shp) == 2 else 0.1
        params[name] = torch.nn.Parameter((torch.randn(*shp, generator=g) * scale).to(cuda))
        offsets.append(off)
        off += (params[name].numel() + 7) // 8 * 8
    flat = torch.zeros(off, dtype=BF, device=cuda)
    for p, o in zip(params.values(), offsets):
        flat[o:o + p.numel()] = p.detach().reshape(-1).to(BF)
    x = (torch.randn(2, T, d, generator=g) * 0.5).to(BF).to(cuda).requires_grad_()
    dy = torch.sin(torch.arange(2 * T * d, dtype=torch.float32)).reshape(2, T, d).to(BF).to(cuda)
    monkeypatch.setattr(Fn, "DGRAD_NN", nn_on)
    Fn.weight_cache.clear()
    Fn.bf16_mirror.attach(flat, list(params.values()), offsets)
    P = params
    y = Fn.linear(x, [P["wa"], P["wb"]], [P["ba"], P["bb"]])                       # [2, T, 128]: the stacked pair, K = 128 = N
    y = Fn.ffn(y, y, SimpleNamespace(weight=P["w1"], bias=P["b1"]), SimpleNamespace(weight=P["w2"], bias=P["b2"]))
    y.backward(dy)
    Fn.flush_wgrads()
    torch.cuda.synchronize()
    return [x.grad] + [p.grad for p in params.values()], Fn.bf16_mirror


def test_mirror_backward_registers_no_transposes_and_keeps_the_gradients(cuda, monkeypatch):
    prev = Fn.compute_dtype()
    Fn.set_compute_dtype(BF)
    try:
        new, mirror = _mirror_backward(cuda, True, monkeypatch)
        assert mirror.flat is not None
        assert not mirror.jobs and mirror.tflat is None, "the data gradients asked for transposed copies"
        old, mirror = _mirror_backward(cuda, False, monkeypatch)
        assert len(mirror.jobs) == 3, "the comparison run did not go through the mirror's transposed copies"
    finally:
        Fn.bf16_mirror.__init__()
        Fn.weight_cache.clear()
        Fn.set_compute_dtype(prev)
    for i, (a, b) in enumerate(zip(new, old)):
        assert a is not None and torch.isfinite(b.float()).all() and b.abs().max().item() > 0, i
        assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)), f"gradient {i} differs from the ST5_DGRAD_NN=0 run"
