"""Pins tests/elementwise_reference.py (no GPU): the fp64 references against torch on the CPU (activations and their autograd
derivatives, index_add_ for the scatters, np.pad(mode="reflect") framing, F.pad for the padded copies, F.cross_entropy and fairseq's
label-smoothed form for the loss), the dropout counter against tests/attention_reference.py, and every emulation's own error against a
cap, so that a bar of 4 x emulation cannot be inflated by a sloppy emulation.

Caps of the emulations (worst element / worst row of |emulation - fp64| / max(|fp64|, 2^-8 largest)): bf16 outputs 2^-8 (one rounding to
an 8-bit significand is 2^-9; a second one, of the fp32 value that straddles a tie, doubles it); fp32 outputs 2^-24 x 64: a handful of
roundings per element, the |x| <= 16 by which the base-2 exp amplifies the rounding of its argument, and the cancellation of
1 + erf(x / sqrt 2) in GELU's lower tail.  The two derivatives that end in 1 - f with f -> 1 (tanh': 1 - t^2; the masking mode of
se_predict: 1 - sigmoid) lose 1 / (1 - f) to that cancellation in any fp32 evaluation of the cited torch expression; the metric's floor
cuts the loss off at 2^8, so their fp32 cap is 2^-24 x 2^8 x 4 = 2^-14."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_reference as A
from tests import elementwise_reference as E
from tests import norm_reference as R

BF, FP = torch.bfloat16, torch.float32
CAP = {BF: 2.0 ** -8, FP: 64 * 2.0 ** -24}
CAP_CANCEL = {BF: 2.0 ** -8, FP: 2.0 ** -14}
TORCH_ACT = {E.ACT_NONE: lambda z: z, E.ACT_GELU: F.gelu, E.ACT_RELU: torch.relu, E.ACT_TANH: torch.tanh,
             E.ACT_LRELU_01: lambda z: F.leaky_relu(z, 0.1), E.ACT_LRELU_001: lambda z: F.leaky_relu(z, 0.01)}


def _close64(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1e-30), (a - b).abs().max().item()


def _vals(n, seed=0, scale=3.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("a", sorted(TORCH_ACT))
def test_activations_equal_torch_and_autograd(a):
    x = _vals(4099)
    xa = x.double().requires_grad_(True)
    y = TORCH_ACT[a](xa)
    dy = _vals(4099, 1, 1.0)
    y.backward(dy.double())
    _close64(E.act_fwd(a, x), y.detach())
    _close64(E.act_bwd(a, dy, x), xa.grad)


@pytest.mark.parametrize("a", sorted(TORCH_ACT))
def test_activations_nonfinite_as_torch(a):
    x = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0])
    want = TORCH_ACT[a](x.double())
    got = E.act(a, x)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.isnan(got[0])                                    # every activation hands a NaN on
    if a != E.ACT_GELU:                                           # (torch's GELU at -inf is NaN on some builds: not a specification)
        assert torch.equal(got[1:], want[1:])
    for dt in (FP, BF):                                           # torch.relu itself hands a NaN on, in both types
        assert torch.isnan(F.relu(torch.tensor([float("nan")], dtype=dt))).all()


@pytest.mark.parametrize("dtype", [BF, FP])
@pytest.mark.parametrize("a", [E.ACT_GELU, E.ACT_TANH])
def test_activation_emulations_are_capped(a, dtype):
    x, dy = E.rounded(_vals(8192), dtype), E.rounded(_vals(8192, 1, 1.0), dtype)
    ref, emu = E.act_fwd(a, x), E.act_fwd(a, x, dtype, True)
    assert 0 < E.flat_errors(emu, ref, ref).max().item() <= CAP[dtype]
    ref, emu = E.act_bwd(a, dy, x), E.act_bwd(a, dy, x, dtype, True)
    assert 0 < E.flat_errors(emu, ref, ref).max().item() <= (CAP_CANCEL if a == E.ACT_TANH else CAP)[dtype]
    # planted faults miss the bar the GPU test uses: a result off by 16 x the cap everywhere, and (fp32) the tanh-approximated GELU
    bad = E.rounded((E.act_fwd(a, x) * (1 + 16 * CAP[dtype])).float(), dtype)
    assert not E.flat_passes(bad[:2055], E.act_fwd(a, x), E.act_fwd(a, x, dtype, True), 2055)[0]
    if a == E.ACT_GELU and dtype == FP:
        assert not E.flat_passes(F.gelu(x, approximate="tanh")[:2055], E.act_fwd(a, x), E.act_fwd(a, x, dtype, True), 2055)[0]
    assert E.flat_passes(E.act_fwd(a, x, dtype, True)[:9], E.act_fwd(a, x), E.act_fwd(a, x, dtype, True), 9)[0]


def test_rounding_bounded_arithmetic_and_its_bounds():
    x, y = _vals(3001), _vals(3001, 1)
    ref, terms = E.axpby(x, y, 0.3, -1.7)
    _close64(ref, float(np.float32(0.3)) * x.double() + float(np.float32(-1.7)) * y.double())
    fp32 = np.float32(0.3) * x + np.float32(-1.7) * y
    assert E.within_b(fp32, ref, terms, 3, FP)[0] and E.within_b(fp32.to(BF), ref, terms, 3, BF)[0]
    assert not E.within_b(fp32 * (1 + 2.0 ** -20), ref, terms, 3, FP)[0]
    assert not E.within_b(torch.full_like(fp32, float("nan")), ref, terms, 3, FP)[0]
    # dropout: the keep set is the counter rule on the flat index; survivors are scaled by 1 / (1 - p)
    keep = E.dropout_keep(77, 0.25, 3001)
    assert torch.equal(keep, torch.from_numpy(R.keep_mask_rows(77, 0.25, 1, 3001))[0])
    assert 0.70 < keep.float().mean().item() < 0.80
    d = E.dropout(x, keep, 0.25)
    _close64(d, x.double() * keep.double() / 0.75)
    for dt in (FP, BF):
        got = E.dropout_bits(E.rounded(x, dt), keep, 0.25, dt)
        assert E.within_b(got, E.dropout(E.rounded(x, dt), keep, 0.25), E.dropout(E.rounded(x, dt), keep, 0.25).abs(), 2, dt)[0]
    assert abs(A.inv_keep(0.25) - 1 / 0.75) < 1e-7
    # sums of squares: the any-order bound holds for an fp32 sum in torch's order and refuses one lost element
    s, mag = E.sumsq(x, 0.5, 3.0)
    assert abs(s - (3.0 + 0.5 * float((x.double() ** 2).sum()))) < 1e-9
    fp = 3.0 + 0.5 * float((x * x).sum())
    assert E.within_d(fp, s, mag, E.sumsq_chain(3001))[0]
    assert not E.within_d(fp - 0.5 * float(x[7] ** 2), s, mag, E.sumsq_chain(3001))[0]
    assert E.sumsq_chain(7) == 8 + 1 + 11 and E.sumsq_chain(7, aligned=False) == 1 + 11
    assert E.sumsq_chain(4194304 + 4099) == 16 + 1 + 11      # the second grid-stride trip
    # se_predict: autograd of sigmoid(x) * src
    src = _vals(3001, 2, 1.0)
    xa = x.double().requires_grad_(True)
    (torch.sigmoid(xa) * src.double()).backward(y.double())
    _close64(E.se_predict_fwd(E.SE_MASKING, x, src), torch.sigmoid(x.double()) * src.double())
    _close64(E.se_predict_bwd(E.SE_MASKING, y, x, src), xa.grad)
    _close64(E.se_predict_fwd(E.SE_DELTA, x, src), x.double() - src.double())
    assert torch.equal(E.se_predict_bwd(E.SE_DELTA, y, x, src), y.double())
    for f, g, cap in ((E.se_predict_fwd(E.SE_MASKING, x, src, True), E.se_predict_fwd(E.SE_MASKING, x, src), CAP[FP]),
                      (E.se_predict_bwd(E.SE_MASKING, y, x, src, True), E.se_predict_bwd(E.SE_MASKING, y, x, src), CAP_CANCEL[FP])):
        assert f.dtype == torch.float32 and 0 < E.flat_errors(f, g, g).max().item() <= cap
    pw = torch.cat([_vals(500).abs() * 1e-6, torch.tensor([0.0, 1e-45, 1e-39, 1e-10, 1.0])])
    _close64(E.log10_floor(pw, 1e-10), torch.log10(torch.clamp(pw.double(), min=float(np.float32(1e-10)))))
    assert E.flat_errors(E.log10_floor(pw, 1e-10, True), E.log10_floor(pw, 1e-10), E.log10_floor(pw, 1e-10)).max().item() <= CAP[FP]
    reim = _vals(6 * 24).view(6, 24)
    mag = E.stft_magnitude(reim, 9, 12)
    _close64(mag[:, :9], torch.complex(reim[:, :9].double(), reim[:, 12:21].double()).abs())
    assert torch.all(mag[:, 9:] == 0)


def test_row_operations_equal_torch():
    g = torch.Generator().manual_seed(3)
    rows, cols, vocab = 37, 20, 11
    x, table, pos = torch.randn(rows, cols, generator=g), torch.randn(vocab, cols, generator=g), torch.randn(50, cols, generator=g)
    tok = torch.randint(0, vocab, (rows,), generator=g, dtype=torch.int32)
    pidx = torch.randint(0, 50, (rows,), generator=g, dtype=torch.int32)
    _close64(E.add_table_rows(x, table, tok, 0.5)[0], x.double() + 0.5 * F.embedding(tok.long(), table.double()))
    _close64(E.embed_rows(table, tok, pos, pidx, 2.0, 0.5)[0], 2.0 * F.embedding(tok.long(), table.double()) + 0.5 * F.embedding(pidx.long(), pos.double()))
    _close64(E.embed_rows(table, tok, None, None, 2.0, 0.0)[0], 2.0 * F.embedding(tok.long(), table.double()))
    # scatter == autograd of the embedding == index_add_, out-of-range ids dropped, row weights applied
    w = table.double().requires_grad_(True)
    (F.embedding(tok.long(), w) * x.double()).sum().backward()
    _close64(E.scatter_rows(x, tok, vocab, 1.0)[0], w.grad)
    t0 = torch.randn(vocab, cols, generator=g)
    bad = tok.clone(); bad[3], bad[8] = -1, vocab + 4
    ok = (bad >= 0) & (bad < vocab)
    rw = torch.tensor([0.5, 2.0, 3.0])
    want = t0.double().index_add_(0, bad[ok].long(), (0.25 * x.double() * rw.double()[(torch.arange(rows) // 4) % 3][:, None])[ok])
    got, mag = E.scatter_rows(x, bad, vocab, 0.25, t0, rw, 4, 3)
    _close64(got, want)
    assert torch.all(mag >= got.abs() - 1e-12)
    assert E.longest_run(torch.tensor([1, 1, 5, -1, -1, -1, 1, 99]), 10) == 3
    # masked fill and its backward
    mask = (torch.rand(rows, generator=g) < 0.4).to(torch.uint8)
    v = torch.randn(cols, generator=g)
    assert torch.equal(E.masked_fill_rows(x, mask, v, FP), torch.where(mask.bool()[:, None], v[None], x))
    xa = x.double().requires_grad_(True)
    va = v.double().requires_grad_(True)
    torch.where(mask.bool()[:, None], va[None], xa).backward(x.double())
    dxr, dv, _ = E.masked_fill_rows_bwd(x, mask)
    _close64(dxr, xa.grad); _close64(dv, va.grad)
    assert E.fill_chain(700) == 3 + 256 + 1 and E.fill_chain(5) == 1 + 5 + 1
    a, b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    for act in (E.ACT_NONE, E.ACT_RELU, E.ACT_TANH, E.ACT_GELU, E.ACT_LRELU_01):
        ref, _ = E.channel_affine(x, a, b, act)
        _close64(ref, TORCH_ACT[act](x.double() * a.double() + b.double()))
        for dt in (FP, BF):
            e = E.channel_affine(E.rounded(x, dt), a, b, act, dt, True)
            assert R.row_metric(e, E.channel_affine(E.rounded(x, dt), a, b, act)[0]) <= CAP[dt]


def test_layouts_equal_torch_and_numpy():
    g = torch.Generator().manual_seed(5)
    src = torch.randn(3, 7, 5, generator=g)
    for pl, pr in ((0, 0), (3, 0), (0, 2), (5, 5)):
        want = F.pad(src, (0, 0, pl, pr))
        assert torch.equal(E.pad_time(src, pl, pr), want)
        assert torch.equal(E.halo_rows(7, pl, pr), (want.abs().sum((0, 2)) == 0))
    live = E.pad_time(src, 2, 1, live=4)
    assert torch.equal(live[:, 2:6], src[:, :4]) and torch.all(live[:, 6:] == 0) and torch.all(live[:, :2] == 0)
    assert torch.equal(E.pad_time(src, 2, 1, live=99), E.pad_time(src, 2, 1)) and torch.all(E.pad_time(src, 2, 1, live=-3) == 0)
    assert E.edge_rows(9, 0, 9).sum() == 0 and E.edge_rows(9, 2, 6).tolist() == [True, True, False, False, False, False, True, True, True]
    # gather3: a permutation and a tap flip are what torch's permute / flip give
    w = torch.randn(4, 6, 5, generator=g)       # [a, b, c]
    idx = E.gather3_index(5, 4, 6, 1, 30, 5, 0)       # dst[c, a, b] = w[a, b, c]
    assert torch.equal(w.reshape(-1)[idx], w.permute(2, 0, 1))
    idx = E.gather3_index(4, 6, 5, 30, 5, -1, 4)      # last axis flipped
    assert torch.equal(w.reshape(-1)[idx], w.flip(2))
    # unfold: the windows a Cin = 1 convolution reads
    wav = torch.randn(2, 400, generator=g)
    u = E.unfold_rows(wav, 10, 5, 16)
    k = torch.randn(1, 1, 10, generator=g)
    assert u.shape == (2 * 79, 16) and torch.all(u[:, 10:] == 0)
    _close64((u[:, :10].double() @ k.double().view(10)).view(2, 79), F.conv1d(wav.double()[:, None], k.double(), stride=5)[:, 0], 1e-12)
    # STFT framing: torch.stft(center=True, pad_mode="reflect") reads exactly these frames
    for S in (9, 10, 33, 64):
        wv = torch.randn(2, S, generator=g)
        fr = E.stft_frames(wv, 16, 4)
        assert fr.shape == (2, 1 + S // 4, 16)
        spec = torch.stft(wv.double(), 16, 4, window=torch.ones(16, dtype=torch.float64), center=True, pad_mode="reflect", return_complex=True)
        _close64(torch.fft.rfft(fr.double(), dim=-1).abs(), spec.abs().transpose(1, 2), 1e-9)
    a, b = torch.randn(8, generator=g), torch.randn(8, generator=g)
    assert E.select(1.0, a, b) is b and E.select(0.0, a, b) is a and E.select(-0.0, a, b) is a


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V", [1, 63, 64, 65])
def test_cross_entropy_equals_torch_and_fairseq(V, eps):
    g = torch.Generator().manual_seed(V)
    rows = 5
    logits = torch.randn(rows, V, generator=g) * 3
    tgt = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)
    tgt[1] = -100 if V > 1 else 0
    ignore = int(tgt[3]) if V > 2 else 7777
    loss, nll, dl = E.cross_entropy(logits, tgt, eps, ignore, 0.5)
    la = logits.double().requires_grad_(True)
    keep = (tgt >= 0) & (tgt != ignore)
    lp = F.log_softmax(la, -1)
    if eps == 0.0:
        want = F.cross_entropy(la[keep], tgt[keep].long(), reduction="sum") if keep.any() else la.sum() * 0
    else:      # fairseq label_smoothed_nll_loss(lprobs, target, epsilon, ignore_index, reduce=True)
        n = -lp.gather(1, tgt.clamp(min=0).long()[:, None])
        s = -lp.sum(-1, keepdim=True)
        n, s = n.masked_fill(~keep[:, None], 0.0), s.masked_fill(~keep[:, None], 0.0)
        eps_i = eps / (V - 1) if V > 1 else 0.0
        want = (1.0 - eps - eps_i) * n.sum() + eps_i * s.sum()
    (0.5 * want).backward()
    assert abs(loss.sum().item() - want.item()) <= 1e-10 * max(1.0, abs(want.item()))
    _close64(dl, la.grad, 1e-10)
    assert torch.all(loss[~keep] == 0) and torch.all(dl[~keep] == 0)
    for dt in (FP, BF):
        lr = E.rounded(logits, dt)
        ref, emu = E.cross_entropy(lr, tgt, eps, ignore, 0.5), E.cross_entropy(lr, tgt, eps, ignore, 0.5, dt, True)
        assert R.row_metric(emu[0], ref[0]) <= CAP[FP] and R.row_metric(emu[1], ref[1]) <= CAP[FP]     # the losses are fp32 in both modes
        assert R.row_metric(emu[2], ref[2]) <= CAP[dt]
