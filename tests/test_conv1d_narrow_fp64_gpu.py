"""csrc/conv1d_narrow.hip (st5_conv1d_narrow: the six direct kernels conv1d_narrow_kernel<CB, NJ>, the two staged ones
conv1d_narrow32_kernel<NJ>; st5_conv1d_cout1) through the C ABI against the fp64 restatement of tests/conv1d_narrow_reference.py.

The bar, per output ELEMENT, nothing in it from a kernel's output (gemm_reference.bar_terms / bar_ratio):
    |kernel - fp64| <= BAR max(|emulation - fp64|, ulp_bf16(fp64) / 2) + summation_floor(S, taps Cin + 16),    BAR = norm_reference.BAR
Every case first asserts, through st5_conv1d_narrow_plan, WHICH kernel it reaches (staged, CB, NJ, tiles per block, tile length, LDS
bytes, against the dispatch restated in the reference), and is judged against the emulation of that form.  The output lies NaN-filled
(or holding the old contents where beta != 0) inside a NaN buffer with GUARD elements behind it; row padding, halo rows, the other
phases of an interleaved output and the gaps between batches must come back bit-identical.  x holds NaN in its row padding, between the
batches and behind the last halo row: none may reach the output.  Everything runs under util.poisoned_allocations().

Lengths per kernel: 1, 15, 16, 17, 31, 32, 33, wave - 1, wave, wave + 1, block - 1, block, block + 1, 2 block + 5 (wave 128 / block 1024 steps;
64 / 512 for Cout = 64), each with B = 1 and B = 3; taps {1, 2, 3, 7, 11} x dilations {1, 3, 5} and the ten epilogue kinds thinned across them.
Each test prints `conv1d-narrow-plan|` and `conv1d-narrow-ratio|` lines (pytest -s); tools/conv1d_narrow_fp64_ratios.py turns those of
an MI355X run into profiles/conv1d_narrow_fp64_ratios.txt."""
import copy
import ctypes
import math

import pytest
import torch
import torch.nn as nn

from speecht5_amd import hip
from tests import conv1d_narrow_reference as C
from tests.util import poisoned_allocations

pytestmark = pytest.mark.gpu

ST5_OK, ST5_ERR_ARG, ST5_ERR_ALIGN = 0, 1, 2
assert (hip.ACT_NONE, hip.ACT_TANH, hip.ACT_LRELU_01, hip.ACT_LRELU_001) == (C.ACT_NONE, C.ACT_TANH, C.ACT_LRELU_01, C.ACT_LRELU_001)


def _on(p, dev):
    """The problem with its buffers on the device."""
    q = copy.copy(p)
    for nm in ("x", "w", "y", "R", "bias"):
        t = getattr(p, nm)
        setattr(q, nm, t.to(dev) if t is not None else None)
    return q


def _abi(p, y):
    """Arguments shared by st5_conv1d_narrow and st5_conv1d_narrow_plan (everything but the last one)."""
    return (p.x.data_ptr() + 2 * p.x_off, p.x_bs, p.x_ts, p.w.data_ptr(), hip.ptr(p.bias), y.data_ptr() + 2 * p.y_off, p.y_bs, p.y_ts,
            p.R.data_ptr() + 2 * p.r_off if p.R is not None else None, p.r_bs, p.r_ts, p.B, p.L, p.Cin, p.Cout, p.taps, p.tap_stride, p.alpha, p.beta,
            p.act)


def _plan(p, y):
    out = (ctypes.c_int32 * 6)(*([-1] * 6))
    rc = hip.lib().st5_conv1d_narrow_plan(*_abi(p, y), ctypes.addressof(out))
    return rc, list(out)


def _kernel_name(pl):
    return f"staged<{pl[2]}>" if pl[0] else f"direct<{pl[1]},{pl[2]}>"


class Ledger:
    def __init__(self):
        self.rows = []

    def add(self, kernel, kind, case, worst, emu_err, touched, nonfinite):
        print(f"conv1d-narrow-ratio|{kernel}|{kind}|{worst:.4f}|{case} (emulation {emu_err:.3e})")
        self.rows.append((kernel, kind, case, worst, touched, nonfinite))

    def settle(self):
        assert self.rows, "nothing was measured"
        missed = [f"{k} {kind} {case}: ratio {w:.3f} (bar {C.BAR}), {t} elements outside the output changed, {n} non-finite outputs"
                  for k, kind, case, w, t, n in self.rows if not w <= C.BAR or t or n]
        assert not missed, f"{len(missed)} misses -- " + "; ".join(missed[:12])


def _launch(p, y):
    if p.Cout == 1:
        return hip.lib().st5_conv1d_cout1(p.x.data_ptr() + 2 * p.x_off, p.x_bs, p.x_ts, p.w.data_ptr(), hip.ptr(p.bias), y.data_ptr(), p.B, p.L, p.Cin,
                                          p.taps, p.tap_stride, p.alpha, p.act, hip.stream())
    return hip.lib().st5_conv1d_narrow(*_abi(p, y), hip.stream())


def _judge(p, y, led, kernel, kind, case, chunk=None):
    """Every output element against the bar and every other element of the y buffer against its initial bits, on the device."""
    worst, emu_err, nonfinite = 0.0, 0.0, 0
    step = chunk or p.B
    for b0 in range(0, p.B, step):
        b1 = min(p.B, b0 + step)
        e = C.expect(p, b0=b0, b1=b1)
        got = y[C.y_offsets(p, b0, b1, y.device)].double()
        nonfinite += int((~torch.isfinite(got)).sum())
        worst, emu_err = max(worst, C.ratio(got, e)), max(emu_err, e.emu_err)
    led.add(kernel, kind, case, worst, emu_err, C.untouched(p, p.y, y), nonfinite)


def _run(p_cpu, dev, led, kind, case, kernel=None):
    """Plan asserted, one launch, judged.  kernel: the kernel the case is meant to reach."""
    p = _on(p_cpu, dev)
    y = p.y.clone()
    rc, pl = _plan(p, y)
    assert rc == ST5_OK and pl == C.plan(p_cpu), (case, rc, pl, C.plan(p_cpu))
    name = _kernel_name(pl)
    assert kernel is None or name == kernel, (case, name, kernel)
    print(f"conv1d-narrow-plan|{name}|tiles_per_block {pl[3]} tile {pl[4]} lds {pl[5]}|{case}")
    hip.check(_launch(p, y), "st5_conv1d_narrow")
    _judge(p, y, led, name, kind, case)
    return name


# ---- the eight kernels at the tile-edge lengths ------------------------------------------------------------------------------------
# kernel -> (Cin, Cout, how the kernel is selected, (taps, dilation) thinned over the lengths)
TD = [(1, 1), (3, 3), (7, 1), (11, 5), (2, 1), (3, 5), (7, 3), (11, 1), (3, 1), (2, 3), (7, 5), (11, 3), (1, 1), (2, 5)]
KERNELS = {
    "staged<2>": (32, 32, {}, TD),
    "staged<4>": (64, 32, {}, [(1, 1), (2, 1), (3, 1), (2, 3), (2, 5)]),           # (everything else at Cin 64 misses the LDS)
    "direct<1,2>": (32, 32, dict(x_pad=8), TD),
    "direct<1,4>": (64, 32, "lds", TD),                                            # (taps <= 3: row padding; beyond: the LDS miss)
    "direct<1,8>": (128, 32, {}, TD),
    "direct<2,2>": (32, 64, {}, TD),
    "direct<2,4>": (64, 64, {}, TD),
    "direct<2,8>": (128, 64, {}, [(t if t < 11 else 9, d) for t, d in TD]),        # (taps 10 is over the LDS limit)
}


def _lengths(CB):
    wave, block = C.WAVE_T[CB], C.TILE_T[CB]
    return [1, 15, 16, 17, 31, 32, 33, wave - 1, wave, wave + 1, block - 1, block, block + 1, 2 * block + 5]


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_each_kernel_at_the_tile_edges(cuda, kernel):
    cin, cout, how, td = KERNELS[kernel]
    led = Ledger()
    with poisoned_allocations():
        for i, (L, B) in enumerate((L, B) for L in _lengths(cout // 32) for B in (1, 3)):
            taps, d = td[i % len(td)]
            kind = C.KINDS[(i + 3 * (cout // 32) + cin // 32) % len(C.KINDS)]
            kw = dict(how) if isinstance(how, dict) else {}
            if kind == "lrelu001":
                if cin > C.LRELU001_MAX_K:
                    kind = "bias_alpha_lrelu01"
                else:
                    taps = min(taps, C.LRELU001_MAX_K // cin)
            if how == "lds" and C.staged_lds(cin, taps, d) <= C.LDS_LIMIT:
                kw = dict(x_pad=8)
            _run(C.case(cin, cout, taps, d, L, B, kind, **kw), cuda, led, kind, f"{cin}->{cout} k{taps} d{d} L{L} B{B} {kw or ''}", kernel)
    led.settle()


def test_every_epilogue_kind_on_both_forms(cuda):
    """The ten kinds on staged<2>, direct<1,2> and direct<2,2> at one ragged length of two time blocks and a half; LRELU_001 also at taps 1
    (the prefetching direct kernels' 'next tap' reloads tap 0) on staged<4>, direct<1,4> and direct<2,4>."""
    led = Ledger()
    with poisoned_allocations():
        for kernel, cin, cout, kw in (("staged<2>", 32, 32, {}), ("direct<1,2>", 32, 32, dict(x_pad=8)), ("direct<2,2>", 32, 64, {})):
            for kind in C.KINDS:
                _run(C.case(cin, cout, 3, 5, 83, 3, kind, **kw), cuda, led, kind, f"{cin}->{cout} k3 d5 L83 B3 {kw or ''}", kernel)
        for kernel, cin, cout, kw in (("staged<4>", 64, 32, {}), ("direct<1,4>", 64, 32, dict(x_pad=8)), ("direct<2,4>", 64, 64, {})):
            _run(C.case(cin, cout, 1, 1, 83, 3, "lrelu001", **kw), cuda, led, "lrelu001", f"{cin}->{cout} k1 d1 L83 B3 {kw or ''}", kernel)
    led.settle()


def test_kernel_selection_edges(cuda):
    """What moves a 32-output-channel call from the staged to the direct form: padded input rows, an output that is only 8-byte aligned
    (y_ts = Cout + 4), and the staged LDS image missing 160 KB (Cin 32: k 11 from d 10 on; Cin 64: from taps 4 at d 1); a padded but
    16-byte-aligned output stays staged.  And the weight image's own limit at Cout 64, Cin 128: taps 9 runs, taps 10 is refused."""
    led = Ledger()
    with poisoned_allocations():
        for cin, taps, d, kw, kernel in ((32, 3, 1, dict(x_pad=8), "direct<1,2>"), (32, 3, 1, dict(y_layout="pad4"), "direct<1,2>"),
                                         (32, 3, 1, dict(y_layout="pad8"), "staged<2>"), (32, 11, 9, {}, "staged<2>"), (32, 11, 10, {}, "direct<1,2>"),
                                         (64, 3, 1, {}, "staged<4>"), (64, 4, 1, {}, "direct<1,4>"), (64, 3, 1, dict(r_pad=4), "direct<1,4>")):
            for L, B in ((33, 3), (1029, 1)):
                _run(C.case(cin, 32, taps, d, L, B, "res_beta", **kw), cuda, led, "res_beta", f"{cin}->32 k{taps} d{d} L{L} B{B} {kw or ''}", kernel)
        _run(C.case(128, 64, 9, 1, 517, 1, "res_beta"), cuda, led, "res_beta", "128->64 k9 d1 L517 B1 (LDS limit)", "direct<2,8>")
        p = _on(C.case(128, 64, 10, 1, 70, 1, "res_beta"), cuda)
        y = p.y.clone()
        assert _plan(p, y)[0] == ST5_ERR_ARG and _launch(p, y) == ST5_ERR_ARG
        torch.cuda.synchronize()
        assert torch.equal(C.bits(y), C.bits(p.y)), "a refused call wrote to y"
    led.settle()


# ---- several tiles per block ----------------------------------------------------------------------------------------------------------
def _device_case(cin, cout, taps, L, B, x_pad, dev):
    """`res_beta` inputs by conv1d_narrow_reference.case's recipe, generated on the device (dilation 1, plain y and R)."""
    g = torch.Generator(device=dev).manual_seed(1000003 * cin + 7919 * cout + L)
    K, rows, x_ts = taps * cin, L + taps - 1, cin + x_pad
    x = torch.full((B * rows * x_ts + C.GUARD,), C.NAN, dtype=C.BF, device=dev)
    x[:B * rows * x_ts].view(B, rows, x_ts)[:, :, :cin] = torch.randn(B, rows, cin, generator=g, device=dev).to(C.BF)
    w = (torch.randn(cout, K, generator=g, device=dev) * (2.0 / math.sqrt(K))).to(C.BF).reshape(-1)
    bias = 1.0 + 0.1 * torch.randn(cout, generator=g, device=dev)
    n = B * L * cout

    def signed(lo, hi, alternate):
        mag = lo + (hi - lo) * torch.rand(B, L, cout, generator=g, device=dev)
        if alternate:
            sign = (1 - 2 * (torch.arange(L, device=dev) % 2)).float().view(1, L, 1)
        else:
            sign = (1 - 2 * torch.randint(0, 2, (B, L, cout), generator=g, device=dev)).float()
        return torch.cat([(mag * sign).to(C.BF).reshape(-1), torch.full((C.GUARD,), C.NAN, dtype=C.BF, device=dev)])
    return C.problem(x, w, signed(2.0, 3.0, False), B, L, cin, cout, taps, x_ts, rows * x_ts, x_ts, L * cout, cout, bias=bias, alpha=0.5, beta=1.0,
                     R=signed(1.0, 1.5, True), r_bs=L * cout, r_ts=cout)


@pytest.mark.parametrize("tiles,tpb", [(3, 2), (5, 4)])
@pytest.mark.parametrize("kernel,cin,cout,x_pad", [("staged<2>", 32, 32, 0), ("direct<1,2>", 32, 32, 8), ("direct<2,2>", 32, 64, 0)])
def test_several_tiles_per_block(cuda, kernel, cin, cout, x_pad, tiles, tpb):
    """B = 1024 with 3 / 5 tiles per batch: 2 / 4 tiles per block, the last block of every batch short.  Inputs generated and every
    element judged on the device, against plain torch float64 operations in chunks of 32 batches."""
    B, L = 1024, (tiles - 1) * C.TILE_T[cout // 32] + 5
    led = Ledger()
    with poisoned_allocations():
        p = _device_case(cin, cout, 3, L, B, x_pad, cuda)
        y = p.y.clone()
        rc, pl = _plan(p, y)
        assert rc == ST5_OK and pl == C.plan(p) and pl[3] == tpb and _kernel_name(pl) == kernel, (rc, pl, C.plan(p))
        print(f"conv1d-narrow-plan|{kernel}|tiles_per_block {pl[3]} tile {pl[4]} lds {pl[5]}|{cin}->{cout} k3 d1 L{L} B{B}")
        hip.check(_launch(p, y), "st5_conv1d_narrow")
        _judge(p, y, led, kernel, f"res_beta tiles_per_block {tpb}", f"{cin}->{cout} k3 d1 L{L} B{B}", chunk=32)
    led.settle()


# ---- one output channel -------------------------------------------------------------------------------------------------------------------
def _run_cout1(p_cpu, dev, led, kind, case):
    p = _on(p_cpu, dev)
    y = p.y.clone()
    print(f"conv1d-narrow-plan|cout1|grid-stride trips {(p.B * p.L + 256 * 16384 - 1) // (256 * 16384)}|{case}")
    hip.check(_launch(p, y), "st5_conv1d_cout1")
    _judge(p, y, led, "cout1", kind, case, chunk=5 if p.B > 5 else None)


def test_cout1(cuda):
    """Taps {1, 7} x Cin {8, 32} x {none, tanh} thinned over L in {1, 255, 256, 257} (one 256-thread block, one output short of and past
    it) x B in {1, 3}, alpha 0.25, half of the cases with padded input rows."""
    led = Ledger()
    combos = [(taps, cin, act) for taps in (1, 7) for cin in (8, 32) for act in (C.ACT_NONE, C.ACT_TANH)]
    with poisoned_allocations():
        i = 0
        for L in (1, 255, 256, 257):
            for B in (1, 3):
                for off in (0, 3):
                    taps, cin, act = combos[(i + off) % len(combos)]
                    x_pad = 8 if (i + off) % 2 else 0
                    _run_cout1(C.cout1_case(cin, taps, L, B, act, x_pad), cuda, led, "tanh" if act == C.ACT_TANH else "none",
                               f"{cin}->1 k{taps} L{L} B{B} x_pad{x_pad}")
                i += 1
    led.settle()


def test_cout1_second_grid_stride_trip(cuda):
    """The grid is capped at 16384 blocks of 256 outputs: B L = 4 194 304 + 96 makes 96 threads take a second trip."""
    B, L = 25, 167776
    assert B * L == 256 * 16384 + 96
    led = Ledger()
    with poisoned_allocations():
        _run_cout1(C.cout1_case(8, 2, L, B, C.ACT_TANH), cuda, led, "tanh", f"8->1 k2 L{L} B{B} (second grid-stride trip)")
    led.settle()


# ---- argument checks ------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(cuda):
    base = _on(C.case(32, 32, 3, 1, 40, 2, "res"), cuda)
    y0 = base.y.clone()

    def rc_of(**kw):
        p = copy.copy(base)
        for k, v in kw.items():
            setattr(p, k, v)
        y = y0.clone()
        rcs = (_plan(p, y)[0], _launch(p, y))
        torch.cuda.synchronize()
        assert torch.equal(C.bits(y), C.bits(y0)), f"a refused call wrote to y: {kw}"
        return rcs
    assert rc_of(act=hip.ACT_TANH) == (ST5_ERR_ARG,) * 2 and rc_of(act=17) == (ST5_ERR_ARG,) * 2          # unknown / unsupported activation
    assert rc_of(r_off=2) == (ST5_ERR_ALIGN,) * 2                                                          # residual 4 bytes off 8-byte alignment
    assert rc_of(y_ts=34) == (ST5_ERR_ALIGN,) * 2 and rc_of(y_bs=40 * 32 + 2) == (ST5_ERR_ALIGN,) * 2     # y strides not multiples of 4
    assert rc_of(r_ts=34) == (ST5_ERR_ALIGN,) * 2
    assert rc_of(y_off=2) == (ST5_ERR_ALIGN,) * 2                                                          # y 4 bytes off 8-byte alignment
    c1 = _on(C.cout1_case(8, 2, 40, 1), cuda)
    y = c1.y.clone()
    for cin in (4, 12):
        c1.Cin = cin
        assert _launch(c1, y) == ST5_ERR_ARG                                                               # cout1: Cin % 8 != 0
    torch.cuda.synchronize()
    assert torch.equal(C.bits(y), C.bits(c1.y))


# ---- through speecht5_amd.hifigan ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def bf16_mode():
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.bfloat16)
    yield
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


@pytest.mark.parametrize("cin,cout,s", [(128, 64, 4), (64, 32, 4), (64, 32, 2), (64, 32, 8)])
def test_wrapper_transposed_conv(cuda, bf16_mode, cin, cout, s):
    """hifigan.conv_transpose1d, every output element against conv_transpose64 under the bar; the emulation and the sum of absolute
    terms behind an element come from the phase problem that owns it."""
    from speecht5_amd import hifigan as H
    led = Ledger()
    B = 2
    with poisoned_allocations():
        for L in (1, 33, 1030):
            x, w, bias = C.transpose_inputs(cin, cout, s, L, B)
            ct = nn.ConvTranspose1d(cin, cout, 2 * s, s, padding=s // 2).to(cuda)
            with torch.no_grad():
                ct.weight.copy_(w)
                ct.bias.copy_(bias)
            y = H.conv_transpose1d(H._pad_act(x.to(cuda).to(C.BF), 1, 1), L, ct)
            assert y.shape == (B, s * L, cout) and y.dtype == C.BF
            got = y.reshape(-1).cpu().double()
            ref = C.conv_transpose64(x, w, bias, s).reshape(-1)
            den, floor = torch.full_like(ref, C.NAN), torch.full_like(ref, C.NAN)
            emu_err = 0.0
            for p in C.transpose_phases(x, w, bias, s):
                e, o = C.expect(p), C.y_offsets(p).reshape(-1)
                assert (e.ref.reshape(-1) - ref[o]).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())
                den[o], floor[o], emu_err = e.den.reshape(-1), e.floor.reshape(-1), max(emu_err, e.emu_err)
                name = _kernel_name(C.plan(p))
            worst = C.G.bar_ratio(got, ref, den, floor).max().item()       # (an element no phase owns has a NaN bar: inf)
            led.add(f"{name} via conv_transpose1d", f"phase s{s}", f"{cin}->{cout} s{s} L{L} B{B}", worst, emu_err, 0,
                    int((~torch.isfinite(got)).sum()))
    led.settle()


def test_wrapper_padded_output_and_odd_stride(cuda, bf16_mode):
    """hifigan.conv1d(..., out_pad): the interior under the bar, the halo rows exactly zero.  conv_transpose1d refuses an odd stride (its
    output of L s rows is the transposed convolution's length only for an even one)."""
    from speecht5_amd import hifigan as H
    led = Ledger()
    B, L, cin, cout, k, d, pad = 2, 1030, 32, 32, 3, 3, 5
    with poisoned_allocations():
        src = C.case(cin, cout, k, d, L, B, "bias_alpha_lrelu01", x_gap=0)
        conv = nn.Conv1d(cin, cout, k, dilation=d, padding=d).to(cuda)
        with torch.no_grad():
            conv.weight.copy_(src.w.float().reshape(cout, k, cin).transpose(1, 2))
            conv.bias.copy_(src.bias)
        xp = src.x[:B * (L + 2 * d) * cin].reshape(B, L + 2 * d, cin).to(cuda)
        yp = H.conv1d(xp, L, conv, alpha=0.5, act=hip.ACT_LRELU_01, out_pad=pad)
        assert yp.shape == (B, L + 2 * pad, cout)
        assert not yp[:, :pad].any() and not yp[:, L + pad:].any(), "halo rows are not exactly zero"
        p = C.problem(src.x, src.w, torch.zeros(B * (L + 2 * pad) * cout, dtype=C.BF), B, L, cin, cout, k, d * cin, (L + 2 * d) * cin, cin,
                      (L + 2 * pad) * cout, cout, y_off=pad * cout, bias=src.bias, alpha=0.5, act=C.ACT_LRELU_01)
        e = C.expect(p)
        got = yp.reshape(-1).cpu()[C.y_offsets(p)].double()
        led.add(f"{_kernel_name(C.plan(p))} via conv1d", "halo", f"{cin}->{cout} k{k} d{d} L{L} B{B} out_pad{pad}", C.ratio(got, e), e.emu_err, 0,
                int((~torch.isfinite(got)).sum()))
        ct = nn.ConvTranspose1d(64, 32, 6, 3, padding=1).to(cuda)
        with pytest.raises(AssertionError):
            H.conv_transpose1d(torch.zeros(1, 6, 64, dtype=C.BF, device=cuda), 4, ct)
    led.settle()
