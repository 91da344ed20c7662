"""tests/conv1d_narrow_reference.py checked on the CPU: the fp64 truth equals torch's own float64 convolutions, the clean emulation of
either form passes the bar, every planted fault fails it, and the inputs of the case generator decide the epilogue faults: the share
of elements on which such a fault would stay under 8 x the element's tolerance is <= 1 % (gemm_reference.mask_decides' condition).
The dispatch restated there (`plan`) is pinned at the edges tests/test_conv1d_narrow_fp64_gpu.py relies on."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv1d_narrow_reference as C

UNDECIDED_CAP = 0.01


def _dense(p, buf, off, bs, ts, rows):
    return buf[C.c_offsets(off, bs, ts, 0, p.B, rows, p.Cin if buf is p.x else p.Cout, "cpu")]


def _torch_conv(p):
    """The same problem through torch.nn.functional.conv1d in float64 on tensors sliced out of the flat buffers."""
    d = p.tap_stride // p.x_ts
    rows = p.L + (p.taps - 1) * d
    x = _dense(p, p.x, p.x_off, p.x_bs, p.x_ts, rows).double().transpose(1, 2)
    w = p.w.double().reshape(p.Cout, p.taps, p.Cin).transpose(1, 2)
    pre = p.alpha * F.conv1d(x, w, None, dilation=d).transpose(1, 2)
    if p.bias is not None:
        pre = pre + p.bias.double()
    if p.Cout == 1:
        v = torch.tanh(pre) if p.act == C.ACT_TANH else pre
    else:
        v = F.leaky_relu(pre, C.G._SLOPE[p.act]) if p.act in C.G._SLOPE else pre
    if p.R is not None:
        v = v + _dense(p, p.R, p.r_off, p.r_bs, p.r_ts, p.L).double()
    if p.beta:
        v = v + p.beta * _dense(p, p.y, p.y_off, p.y_bs, p.y_ts, p.L).double()
    return v


TRUTH_CASES = [(32, 32, 3, 1, 70, 2, "plain", {}), (32, 32, 11, 5, 33, 3, "bias_alpha_lrelu01", {}), (32, 32, 2, 3, 40, 2, "lrelu001", dict(x_pad=8)),
               (128, 64, 2, 1, 17, 2, "res_beta", {}), (64, 64, 1, 1, 65, 1, "res_strided", {}), (32, 64, 3, 5, 31, 3, "beta05", dict(y_layout="pad4")),
               (32, 32, 3, 3, 50, 2, "halo", {}), (64, 32, 2, 1, 50, 2, "phase", {})]


@pytest.mark.parametrize("cin,cout,taps,d,L,B,kind,kw", TRUTH_CASES)
def test_truth_equals_torch_float64(cin, cout, taps, d, L, B, kind, kw):
    p = C.case(cin, cout, taps, d, L, B, kind, **kw)
    ref, want = C.conv(p).y, _torch_conv(p)
    assert torch.isfinite(ref).all()
    assert (ref - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("act", [C.ACT_NONE, C.ACT_TANH])
def test_cout1_truth_equals_torch_float64(act):
    p = C.cout1_case(32, 7, 257, 3, act=act, x_pad=8)
    assert (C.conv(p).y - _torch_conv(p)).abs().max().item() <= 1e-12


@pytest.mark.parametrize("cin,cout,s,L,B", [(128, 64, 4, 33, 2), (64, 32, 2, 1, 1), (64, 32, 8, 9, 2)])
def test_transposed_restatement_equals_torch_float64(cin, cout, s, L, B):
    x, w, bias = C.transpose_inputs(cin, cout, s, L, B)
    ref = C.conv_transpose64(x, w, bias, s)
    want = F.conv_transpose1d(x.double().transpose(1, 2), w.double(), bias.double(), stride=s, padding=s // 2).transpose(1, 2)
    assert ref.shape == (B, s * L, cout) and (ref - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    # ... and the phase problems (what the wrapper launches) add up to it: every output element belongs to exactly one phase
    img = torch.full((B * L * s * cout,), float("nan"), dtype=torch.float64)
    for p in C.transpose_phases(x, w, bias, s):
        img[C.y_offsets(p).reshape(-1)] = C.conv(p).y.reshape(-1)
    assert (img.view(B, s * L, cout) - ref).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


BAR_CASES = [(32, 32, 3, 1, 70, 2, kind, {}) for kind in C.KINDS] + \
            [(64, 64, 7, 3, 70, 2, kind, {}) for kind in C.KINDS if kind != "lrelu001"] + [(64, 64, 1, 1, 70, 2, "lrelu001", {})] + \
            [(32, 32, 3, 1, 70, 2, kind, dict(x_pad=8)) for kind in ("bias_alpha_lrelu01", "lrelu001", "res_beta")] + \
            [(128, 32, 11, 5, 33, 1, "res_beta", {}), (128, 64, 9, 1, 33, 1, "bias_alpha_lrelu01", {}), (64, 32, 1, 1, 33, 1, "lrelu001", {})]


@pytest.mark.parametrize("cin,cout,taps,d,L,B,kind,kw", BAR_CASES)
def test_clean_emulation_passes_the_bar(cin, cout, taps, d, L, B, kind, kw):
    p = C.case(cin, cout, taps, d, L, B, kind, **kw)
    forms = ("direct",) if cout == 64 or kw or cin == 128 else ("direct", "staged")
    assert C.form_of(p) == forms[-1]
    for form in forms:
        e = C.expect(p, form)
        r = C.ratio(e.emu, e)
        assert r <= 1.0 + 1e-9, (form, r)       # (the emulation's own error is the bar's yardstick: its ratio is at most 1)
        assert 0 < e.emu_err < 0.05


def _fault_case(fault, cout):
    cin = 64 if cout == 64 else 32
    if fault == "phase_t_off":
        x, w, bias = C.transpose_inputs(cin, cout, 4, 70, 2)
        return C.transpose_phases(x, w, bias, 4)[1]
    kind = {"bias_before_alpha": "bias_alpha_lrelu01", "slope_01": "lrelu001", "r_row": "res", "beta_ignored": "beta05", "y_bs_dense": "halo"}.get(fault, "res_beta")
    return C.case(32 if fault == "slope_01" else cin, cout, 3, 3, 70, 2, kind)


@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("fault", C.FAULTS)
def test_every_planted_fault_fails_the_bar(fault, cout):
    p = _fault_case(fault, cout)
    e = C.expect(p)
    bad = C.conv(p, emulate=True, fault=fault).y
    r = C.G.bar_ratio(bad, e.ref, e.den, e.floor)
    assert r.max().item() > 8 * C.BAR, (fault, r.max().item())
    assert C.ratio(e.emu, e) <= 1.0 + 1e-9


def test_cout1_dropped_tap_fails_the_bar():
    p = C.cout1_case(8, 7, 257, 3)
    e = C.expect(p)
    assert e.form == "cout1" and C.ratio(e.emu, e) <= 1.0 + 1e-9
    assert C.ratio(C.conv(p, emulate=True, fault="last_tap_dropped").y, e) > 8 * C.BAR


DECIDE_KINDS = {"bias_before_alpha": ("bias_alpha_lrelu01",), "slope_01": ("lrelu001",), "r_row": ("res", "res_strided", "res_beta"),
                "beta_ignored": ("beta1", "beta05", "res_beta")}


DECIDE_SHAPES = [(32, 32, 3, 1), (32, 32, 11, 5), (64, 32, 7, 3), (128, 32, 2, 1), (32, 64, 1, 1), (64, 64, 7, 3), (128, 64, 9, 1)]
LRELU001_SHAPES = [(32, 32, 1, 1), (32, 32, 3, 5), (32, 32, 2, 3), (64, 32, 1, 1), (32, 64, 3, 1), (32, 64, 2, 3), (64, 64, 1, 1)]     # (every one the GPU test uses)


@pytest.mark.parametrize("fault,cin,cout,taps,d", [(f,) + s for f in C.EPILOGUE_FAULTS for s in (LRELU001_SHAPES if f == "slope_01" else DECIDE_SHAPES)])
def test_inputs_decide_the_epilogue_faults(fault, cin, cout, taps, d):
    for kind in DECIDE_KINDS[fault]:
        p = C.case(cin, cout, taps, d, 130, 3, kind)
        for form in {"direct", C.form_of(p)}:
            e = C.expect(p, form)
            share, n = C.decides(p, e, fault, form)
            assert n >= 0.05 * e.ref.numel(), (kind, n)          # (slope_01: enough negative pre-activations to speak of)
            assert share <= UNDECIDED_CAP, (fault, kind, form, share)


def test_plan_restated_at_the_lds_edges():
    pl = lambda *a, **k: C.plan(C.case(*a, **k))
    assert pl(32, 32, 3, 1, 40, 1)[:3] == [1, 1, 2] and pl(64, 32, 3, 1, 40, 1)[:3] == [1, 1, 4]
    assert pl(32, 32, 3, 1, 40, 1, x_pad=8)[0] == 0 and pl(32, 32, 3, 1, 40, 1, y_layout="pad4")[0] == 0 and pl(32, 32, 3, 1, 40, 1, y_layout="pad8")[0] == 1
    assert pl(32, 32, 11, 9, 40, 1)[0] == 1 and pl(32, 32, 11, 10, 40, 1)[0] == 0           # 162 560 / 168 960 bytes against 163 840: d = 10 is over
    assert C.staged_lds(32, 11, 9) <= C.LDS_LIMIT < C.staged_lds(32, 11, 10)
    assert pl(64, 32, 3, 1, 40, 1)[0] == 1 and pl(64, 32, 4, 1, 40, 1)[0] == 0 and pl(64, 32, 3, 2, 40, 1)[0] == 0
    assert pl(128, 32, 3, 1, 40, 1)[:3] == [0, 1, 8] and pl(128, 64, 9, 1, 40, 1)[:3] == [0, 2, 8]
    assert 64 * (9 * 128 + 8) * 2 <= C.LDS_LIMIT < 64 * (10 * 128 + 8) * 2
    assert C.tiles_per_block(1024, 2 * 1024 + 5, 1) == 2 and C.tiles_per_block(1024, 4 * 1024 + 5, 1) == 4
    assert C.tiles_per_block(1024, 2 * 512 + 5, 2) == 2 and C.tiles_per_block(1024, 4 * 512 + 5, 2) == 4 and C.tiles_per_block(3, 2053, 1) == 1


def _library_plan(p, x=0x100000, w=0x200000, y=0x300000, r=0x400000):
    """st5_conv1d_narrow_plan on made-up, 16-byte-aligned addresses (host only: the query dereferences nothing)."""
    import ctypes
    from speecht5_amd import hip
    out = (ctypes.c_int32 * 6)(*([-1] * 6))
    rc = hip.lib().st5_conv1d_narrow_plan(x + 2 * p.x_off, p.x_bs, p.x_ts, w, 0x500000 if p.bias is not None else None, y + 2 * p.y_off, p.y_bs, p.y_ts,
                                          r + 2 * p.r_off if p.R is not None else None, p.r_bs, p.r_ts, p.B, p.L, p.Cin, p.Cout, p.taps, p.tap_stride,
                                          p.alpha, p.beta, p.act, ctypes.addressof(out))
    return rc, list(out)


def test_library_plan_equals_the_restatement():
    """The built library's plan query (no GPU needed) against `plan`: every kernel, both sides of every selection edge, the tiles per
    block of a B = 1024 batch, and the error codes of what the launch refuses."""
    import copy
    seen = set()
    cases = [(cin, cout, taps, d, {}) for cin in (32, 64, 128) for cout in (32, 64) for taps, d in ((1, 1), (3, 1), (2, 5), (2, 6), (2, 7), (4, 1), (3, 2), (9, 1), (11, 9), (11, 10))
             if cout * (taps * cin + 8) * 2 <= C.LDS_LIMIT]
    cases += [(32, 32, 3, 1, kw) for kw in (dict(x_pad=8), dict(y_layout="pad4"), dict(y_layout="pad8"), dict(r_pad=4), dict(r_pad=8), dict(y_layout="phase"), dict(y_layout="halo"))]
    for cin, cout, taps, d, kw in cases:
        p = C.case(cin, cout, taps, d, 40, 2, "res_beta", **kw)
        rc, pl = _library_plan(p)
        assert rc == 0 and pl == C.plan(p), (cin, cout, taps, d, kw, rc, pl, C.plan(p))
        seen.add(tuple(pl[:3]))
        if pl[0]:          # an output or residual that is 8- but not 16-byte aligned: the direct form
            assert _library_plan(p, y=0x300008)[1][0] == 0 and _library_plan(p, r=0x400008)[1][0] == 0
    assert seen == {(1, 1, 2), (1, 1, 4), (0, 1, 2), (0, 1, 4), (0, 1, 8), (0, 2, 2), (0, 2, 4), (0, 2, 8)}
    for cout, x_pad in ((32, 0), (32, 8), (64, 0)):
        for tiles, tpb in ((3, 2), (5, 4), (9, 8), (17, 8)):
            p = C.case(32, cout, 3, 1, 40, 1, "res_beta", x_pad=x_pad)
            p.B, p.L = 1024, (tiles - 1) * C.TILE_T[cout // 32] + 5          # (only the numbers matter to the query)
            rc, pl = _library_plan(p)
            assert rc == 0 and pl == C.plan(p) and pl[3] == tpb and pl[4] == C.TILE_T[cout // 32], (cout, x_pad, tiles, pl)
    base = C.case(32, 32, 3, 1, 40, 2, "res")

    def rc_of(addr=None, **kw):
        p = copy.copy(base)
        for k, v in kw.items():
            setattr(p, k, v)
        return _library_plan(p, **(addr or {}))[0]
    assert rc_of() == 0
    assert rc_of(act=C.ACT_TANH) == 1 and rc_of(act=17) == 1 and rc_of(Cout=48) == 1 and rc_of(Cin=24) == 1 and rc_of(L=0) == 1
    assert rc_of(r_off=2) == 2 and rc_of(y_off=2) == 2 and rc_of(y_ts=34) == 2 and rc_of(y_bs=1282) == 2 and rc_of(r_ts=34) == 2 and rc_of(x_ts=36) == 2
    assert rc_of(addr=dict(x=0x100008)) == 2 and rc_of(addr=dict(w=0x200008)) == 2
    assert _library_plan(C.case(128, 64, 9, 1, 40, 1))[0] == 0 and _library_plan(C.case(128, 64, 10, 1, 40, 1))[0] == 1
