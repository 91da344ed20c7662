"""The CTC loss (csrc/ctc_loss.hip through functional.ctc_loss_sum and the C ABI) and the CTC prefix scorer of joint CTC /
attention beam search (csrc/ctc_prefix.hip through sequence_generator.CTCPrefixScorer) at ASR recipe shapes, against the fp64
references of tests/ctc_reference.py, which tests/test_ctc_reference_cpu.py pins to brute force.

Recipe shapes: the character vocabulary of 83 symbols with <ctc_blank> last (blank = 82; blank = 0 too), up to 1750 encoder
frames (35 s at 50 frames / s) and 600 labels, i.e. 2 L + 1 = 1201 states, 4.7 passes of the 256-thread block.  Target lengths
31 / 32 / 127 / 128 / 255 / 256 / 600 put the last state on either side of the wave (64) and block (256) boundaries.

Error model.  fp32 log-space alpha / beta rows cannot do better than torch's own fp32 CTC: the posterior is
exp(log sum + mx + nll - lp) with mx ~ -nll in the thousands, so the gradient error grows with the length (about 1e-2 of
max |g| at 1750 frames, 600 labels).  Every case therefore runs torch's fp32 CPU CTC on the same inputs and holds the kernel to
K = 4 times torch's error against fp64, plus a floor (2e-7 relative for the nll, 1e-6 max |g| for gradients).  Measured on an
MI355X, kernel error / torch-fp32 error over the cases: nll 1.00 in every case, gradient 0.88-1.04, gradient through the
log-softmax 0.89-1.04; the gradient error itself reached 1.0e-2 max |g| at 1750 frames and 1.9e-2 at the LDS limit (1908
labels).  The prefix scorer is held the same way to the fp32 numpy restatement of the reference's arithmetic: ratio 1.00.

Every buffer the product allocates is poisoned (tests.util.poisoned_allocations) and the C ABI calls write into NaN-filled
buffers, so an output the kernels skip shows up as NaN."""
import collections

import numpy as np
import pytest
import torch

from speecht5_amd import functional as Fn
from speecht5_amd import hip
from speecht5_amd.sequence_generator import CTCPrefixScorer
from tests.ctc_reference import LOGZERO, ctc_loss_ref, prefix_initial, prefix_score
from tests.util import poisoned_allocations

pytestmark = pytest.mark.gpu

V = 83
K = 4.0               # kernel error <= K x the fp32 reference's error (+ floor)
REL_FLOOR = 2e-7      # nll / prefix scores: relative to the magnitude
GRAD_FLOOR = 1e-6     # gradients: relative to max |g|
ST5_ERR_ARG = 1
LDS_CAP_WORDS = 60 * 1024 // 4


def min_frames(tg):
    """Fewest frames that can emit `tg`: one per label, plus a blank between two equal neighbours."""
    return len(tg) + sum(1 for a, b in zip(tg, tg[1:]) if a == b)


def make_target(rng, L, blank, style):
    labels = np.array([c for c in range(V) if c != blank])
    if style == "random":   # 60 of the 82 classes: the others never appear
        return [int(c) for c in rng.choice(rng.choice(labels, 60, replace=False), L)]
    # "runs": one dominant class in runs of 20..120 (hundreds of positions in the class-sorted list; the l'_s != l'_{s-2}
    # rule fires at every repeat), between short runs of 4 others
    pool = rng.choice(labels, 5, replace=False)
    out = []
    while len(out) < L:
        out += [int(pool[0])] * int(rng.randint(20, 121))
        out += [int(rng.choice(pool[1:]))] * int(rng.randint(1, 4))
    return out[:L]


Case = collections.namedtuple("Case", "id T blank regime style lens tbs zi gout maxL")
TIGHT = [200, 200, 128, 31, 1, 0, 0, 2]
TIGHT_TB = ["tight", "short", "tight", "short", 1, 1, 0, 0]
CASES = [
    Case("T499-b82-flat", 499, 82, "flat", "random", [31, 32, 127, 128, 255, 256, 200, 0], [499, 498, 400, 350, 499, 300, 260, 17],
         True, 1.0, 300),
    Case("T499-b0-peaked", 499, 0, "peaked", "random", [256, 255, 128, 127, 32, 31, 0, 200], [499, 470, 333, 499, 120, 40, 9, 400],
         True, 0.37, None),
    Case("T1750-b82-flat", 1750, 82, "flat", "random", [600, 256, 255, 128, 127, 32, 31, 600], [1750, 1700, 1200, 900, 1749, 400, 64, 1500],
         True, -0.5, 640),
    Case("T1750-b0-peaked", 1750, 0, "peaked", "random", [600, 600, 31, 32, 127, 128, 255, 256], [1750, 1400, 1750, 77, 1000, 500, 700, 1600],
         True, 1.0, None),
    Case("T1750-b82-runs-flat", 1750, 82, "flat", "runs", [600, 256, 128, 600], [1750, 1600, 1200, 1300], True, 0.37, None),
    Case("T1750-b0-runs-peaked", 1750, 0, "peaked", "runs", [600, 255, 600, 127], [1750, 900, 1500, 600], True, -1.0, 700),
    Case("T499-b82-tight-zi", 499, 82, "flat", "runs", TIGHT, TIGHT_TB, True, 1.0, None),
    Case("T499-b0-tight-peaked-nozi", 499, 0, "peaked", "runs", TIGHT, TIGHT_TB, False, 0.37, None),
    Case("T499-b82-tight-peaked-nozi", 499, 82, "peaked", "random", TIGHT, TIGHT_TB, False, -2.0, 256),
    Case("T499-b82-empty", 499, 82, "flat", "random", [0] * 8, [499, 1, 0, 250, 498, 2, 100, 499], True, 1.0, 0),
]


def build(case, seed):
    """-> targets (list of lists), input lengths [B], fp32 logits [T, B, V] (peaked: +10 on one alignment of each feasible
    sentence, so the nll is small; flat: N(0, 2^2), nll in the thousands at 1750 frames)."""
    rng = np.random.RandomState(seed)
    tgs = [make_target(rng, L, case.blank, case.style) for L in case.lens]
    tbs = []
    for tg, tb in zip(tgs, case.tbs):
        if tb == "tight":
            tb = min_frames(tg)
        elif tb == "short":
            tb = min_frames(tg) - 1
        else:
            assert tb == 0 or tb >= min_frames(tg), (case.id, tb, min_frames(tg))
        assert 0 <= tb <= case.T
        tbs.append(tb)
    B = len(tgs)
    x = rng.randn(case.T, B, V) * (2.0 if case.regime == "flat" else 1.0)
    if case.regime == "peaked":
        for b, (tg, tb) in enumerate(zip(tgs, tbs)):
            if tb < min_frames(tg):
                continue
            seq = []
            for i, c in enumerate(tg):
                if i and tg[i - 1] == c:
                    seq.append(case.blank)
                seq.append(c)
            seq = seq or [case.blank]
            for t in range(tb):   # stretch the shortest emission over the frames: collapses to tg
                x[t, b, seq[t * len(seq) // tb]] += 10.0
    return tgs, torch.tensor(tbs, dtype=torch.long), torch.tensor(x, dtype=torch.float32)


def flat_targets(tgs):
    return torch.tensor([c for t in tgs for c in t], dtype=torch.long), torch.tensor([len(t) for t in tgs], dtype=torch.long)


def abi_fwd(lp, flat, in_len, tg_len, maxL, blank, zi):
    """st5_ctc_loss_fwd into NaN-filled nll / loss / workspace; -> (rc, nll, loss, ws, device index tensors)."""
    T, B, v = lp.shape
    dev = lp.device
    flat, in_len, tg_len = flat.to(dev), in_len.to(dev), tg_len.to(dev)
    offsets = torch.cumsum(tg_len, 0) - tg_len
    nll = torch.full((B,), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    ws = torch.full((max(int(hip.lib().st5_ctc_loss_ws_bytes(T, B, maxL)), 4) // 4,), float("nan"), device=dev)
    rc = hip.lib().st5_ctc_loss_fwd(lp.data_ptr(), hip.ptr(flat) if flat.numel() else 0, offsets.data_ptr(), in_len.data_ptr(),
                                    tg_len.data_ptr(), T, B, v, maxL, blank, int(zi), nll.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                    hip.stream())
    return rc, nll, loss, ws, (flat, offsets, in_len, tg_len)


def abi_bwd(lp, idx, maxL, blank, zi, nll, gout, ws):
    """st5_ctc_loss_bwd into a NaN-filled gradient; -> (rc, grad)."""
    T, B, v = lp.shape
    flat, offsets, in_len, tg_len = idx
    g = torch.tensor([gout], dtype=torch.float32, device=lp.device)
    grad = torch.full_like(lp, float("nan"))
    rc = hip.lib().st5_ctc_loss_bwd(lp.data_ptr(), hip.ptr(flat) if flat.numel() else 0, offsets.data_ptr(), in_len.data_ptr(),
                                    tg_len.data_ptr(), T, B, v, maxL, blank, int(zi), nll.data_ptr(), g.data_ptr(), ws.data_ptr(),
                                    grad.data_ptr(), hip.stream())
    return rc, grad


def max_err(a, b, cols=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if cols is not None:
        a, b = a[:, cols], b[:, cols]
    return float((a - b).abs().max()) if a.numel() else 0.0


def check_ctc(case_id, lp, x_grad, lp_grad, nll_k, loss_k, tgs, in_len, flat, tg_len, blank, zi, gout, logits):
    """Loss, per-sentence nll and both gradients of one run against fp64, under the torch-fp32 error model.  -> ratios."""
    T, B, _ = lp.shape
    r64 = ctc_loss_ref(lp, flat, in_len, tg_len, blank, zi, gout, logits=logits, dtype=torch.float64)
    r32 = ctc_loss_ref(lp, flat, in_len, tg_len, blank, zi, gout, logits=logits, dtype=torch.float32)
    possible = [tb >= min_frames(tg) for tg, tb in zip(tgs, in_len.tolist())]
    nll_k = nll_k.double().cpu()
    # per sentence: every sentence within K x torch's worst relative error of this case
    scale = r64["nll"].abs().clamp_min(1.0)
    ok = torch.tensor(possible)
    e_t = float(((r32["nll"].double() - r64["nll"]).abs() / scale)[ok].max()) if ok.any() else 0.0
    e_k = ((nll_k - r64["nll"]).abs() / scale)[ok]
    assert (e_k <= K * e_t + REL_FLOOR).all(), (case_id, e_k.tolist(), e_t)
    assert torch.isinf(nll_k[~ok]).all(), (case_id, nll_k[~ok])   # the kernel's nll stays inf; zero_infinity acts in the sum
    # the sum: exact summation of per-sentence errors is bounded by their sum (the kernel sums in fp64)
    if zi or all(possible):
        sum_t = float((r32["nll"].double() - r64["nll"]).abs().sum())
        e_loss = abs(float(loss_k) - float(r64["loss"]))
        assert e_loss <= K * sum_t + REL_FLOOR * abs(float(r64["loss"])), (case_id, e_loss, sum_t, float(r64["loss"]))
    else:
        assert float(loss_k) == float("inf")
    # gradients: all sentences except the impossible ones without zero_infinity (torch's gradient there is NaN)
    cols = [b for b in range(B) if possible[b] or zi]
    assert not torch.isnan(lp_grad).any() and not torch.isnan(x_grad).any()
    ratios = dict(nll=float(e_k.max()) / e_t if e_t > 0 and len(e_k) else 0.0)
    for name, got, key in (("grad", lp_grad, "grad"), ("grad_logits", x_grad, "grad_logits")):
        ek, et = max_err(got, r64[key], cols), max_err(r32[key], r64[key], cols)
        sc = float(r64[key][:, cols].abs().max()) if cols else 0.0
        assert ek <= K * et + GRAD_FLOOR * sc, (case_id, name, ek, et, sc)
        ratios[name] = ek / et if et > 0 else 0.0
        ratios[name + "_rel"] = ek / sc if sc > 0 else 0.0
    print(f"{case_id}: " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    return ratios


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_ctc_loss_recipe_shapes(cuda, case):
    """Fn.ctc_loss_sum forward + backward, the gradient w.r.t. lprobs and through the log-softmax in front (as the ASR criterion
    computes it), and the per-sentence nll of st5_ctc_loss_fwd, against fp64."""
    tgs, in_len, logits = build(case, seed=sum(map(ord, case.id)))
    flat, tg_len = flat_targets(tgs)
    maxL = case.maxL if case.maxL is not None else int(tg_len.max())
    T, B, _ = logits.shape
    x = logits.to(cuda).requires_grad_(True)
    with poisoned_allocations():
        lp = torch.log_softmax(x, -1)
        lp.retain_grad()
        loss = Fn.ctc_loss_sum(lp, flat.to(cuda), in_len.to(cuda), tg_len.to(cuda), case.blank, case.zi, max_target_len=maxL)
        (loss * case.gout).backward()
        rc, nll, loss2, _, _ = abi_fwd(lp.detach(), flat, in_len, tg_len, maxL, case.blank, case.zi)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(loss.detach().reshape(1), loss2)
    g = lp.grad.cpu()
    for b in range(B):   # frames past a sentence's length take no gradient
        assert torch.equal(g[int(in_len[b]):, b], torch.zeros(T - int(in_len[b]), V))
    check_ctc(case.id, lp.detach().cpu(), x.grad, g, nll, loss.detach(), tgs, in_len, flat, tg_len, case.blank, case.zi, case.gout,
              logits)


@pytest.mark.parametrize("zi", [True, False], ids=["zi", "nozi"])
def test_ctc_loss_writes_every_output(cuda, zi):
    """st5_ctc_loss_fwd / _bwd once through the C ABI into NaN-filled buffers: ragged lengths, a sentence one frame short of
    its labels (zeroed by zero_infinity), T_b = 1 and T_b = 0.  Frames t >= T_b come out exactly 0, every frame of a zeroed
    sentence too, and nothing is left NaN."""
    case = CASES[6]._replace(zi=zi)
    tgs, in_len, logits = build(case, seed=11)
    flat, tg_len = flat_targets(tgs)
    maxL = int(tg_len.max()) + 3
    lp = torch.log_softmax(logits, -1).to(cuda)
    rc, nll, loss, ws, idx = abi_fwd(lp, flat, in_len, tg_len, maxL, case.blank, zi)
    assert rc == 0
    rc, grad = abi_bwd(lp, idx, maxL, case.blank, zi, nll, 0.37, ws)
    assert rc == 0
    torch.cuda.synchronize()
    nll, loss, grad = nll.cpu(), loss.cpu(), grad.cpu()
    assert not torch.isnan(nll).any() and not torch.isnan(loss).any() and not torch.isnan(grad).any()
    dead = [b for b, (tg, tb) in enumerate(zip(tgs, in_len.tolist())) if tb < min_frames(tg)]
    assert dead == [1, 3, 7]
    for b in range(len(tgs)):
        tb = 0 if (zi and b in dead) else int(in_len[b])
        assert torch.equal(grad[tb:, b], torch.zeros(case.T - tb, V)), b
        assert tb == 0 or bool((grad[:tb, b] != 0).any()), b
    assert torch.isinf(nll[dead]).all() and bool(torch.isfinite(loss).all()) == zi


def test_ctc_loss_deterministic(cuda):
    """Two runs of forward + backward: bitwise-equal nll, loss and gradient."""
    case = CASES[2]
    tgs, in_len, logits = build(case, seed=3)
    flat, tg_len = flat_targets(tgs)
    lp = torch.log_softmax(logits, -1).to(cuda)
    outs = []
    for _ in range(2):
        rc, nll, loss, ws, idx = abi_fwd(lp, flat, in_len, tg_len, case.maxL, case.blank, True)
        assert rc == 0
        rc, grad = abi_bwd(lp, idx, case.maxL, case.blank, True, nll, -0.5, ws)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((nll.cpu(), loss.cpu(), grad.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def max_target_len_accepted(v):
    """The largest max_target_len both passes accept: the backward's LDS rows, (8 maxL + V + 12) words, in 60 KiB."""
    return (LDS_CAP_WORDS - 12 - v) // 8


def test_ctc_loss_lds_limit(cuda):
    """Forward and backward at the largest max_target_len the library accepts for V = 83 (1908 labels, 3817 states, 15 passes of
    the block) against fp64; one label more is refused by BOTH passes before any kernel runs, and by the autograd forward
    (never half-way through a training step, in the backward).  The bound at V = 1024 is refused the same way."""
    L = max_target_len_accepted(V)
    assert L == 1908
    rng = np.random.RandomState(17)
    tgs = [make_target(rng, L, V - 1, "random"), make_target(rng, 1000, V - 1, "random")]
    in_len = torch.tensor([min_frames(tgs[0]) + 40, min_frames(tgs[1]) + 500])
    T = int(in_len.max()) + 5
    flat, tg_len = flat_targets(tgs)
    logits = torch.tensor(rng.randn(T, 2, V) * 2.0, dtype=torch.float32)
    x = logits.to(cuda).requires_grad_(True)
    with poisoned_allocations():
        lp = torch.log_softmax(x, -1)
        lp.retain_grad()
        loss = Fn.ctc_loss_sum(lp, flat.to(cuda), in_len.to(cuda), tg_len.to(cuda), V - 1, True, max_target_len=L)
        loss.backward()
        rc, nll, _, _, _ = abi_fwd(lp.detach(), flat, in_len, tg_len, L, V - 1, True)
    assert rc == 0
    torch.cuda.synchronize()
    check_ctc("lds-limit", lp.detach().cpu(), x.grad, lp.grad.cpu(), nll, loss.detach(), tgs, in_len, flat, tg_len, V - 1, True, 1.0,
              logits)
    # one label more: refused by both entries, nothing launched (the NaN-filled outputs stay NaN)
    for v in (V, 1024):
        lpv = torch.log_softmax(torch.zeros(T, 2, v, device=cuda), -1)
        over = max_target_len_accepted(v) + 1
        rc, nll, loss, ws, idx = abi_fwd(lpv, flat, in_len, tg_len, over, v - 1, True)
        assert rc == ST5_ERR_ARG, (v, rc)
        rc, grad = abi_bwd(lpv, idx, over, v - 1, True, nll, 1.0, ws)
        assert rc == ST5_ERR_ARG, (v, rc)
        torch.cuda.synchronize()
        assert torch.isnan(nll).all() and torch.isnan(loss).all() and torch.isnan(grad).all()
    xr = logits.to(cuda).requires_grad_(True)
    with pytest.raises(hip.HipKernelError, match="st5_ctc_loss_fwd"):
        Fn.ctc_loss_sum(torch.log_softmax(xr, -1), flat.to(cuda), in_len.to(cuda), tg_len.to(cuda), V - 1, True, max_target_len=L + 1)


# ------------------------------------------------------------------------------------------------------------------------------
# prefix scorer
# ------------------------------------------------------------------------------------------------------------------------------
NH, BLANK, EOS = 10, V - 1, 2   # 2 sentences x beam 5; <ctc_blank> last, </s> = 2 as in the dictionaries


def check_log_space(what, got, r64, r32):
    """got (kernel), r32 (fp32 restatement) against r64, split by the fp64 value into real log-probabilities and LOGZERO-derived
    sentinels (fp32 cannot resolve a sum near -1e10, so both fp32 forms stay at -1e10 where fp64 drifts): in each part the
    kernel's max error <= K x the fp32 restatement's + REL_FLOOR x the part's magnitude.  -> ratio in the real part."""
    got, r64, r32 = (np.asarray(a, dtype=np.float64) for a in (got, r64, r32))
    assert np.isfinite(got).all(), what
    ratios = []
    for part in (r64 > LOGZERO / 2, r64 <= LOGZERO / 2):
        if not part.any():
            ratios.append(0.0)
            continue
        ek, et = np.abs(got - r64)[part].max(), np.abs(r32 - r64)[part].max()
        sc = np.abs(r64[part]).max()
        assert ek <= K * et + REL_FLOOR * sc, (what, ek, et, sc)
        ratios.append(ek / et if et > 0 else 0.0)
    return ratios[0]


def synthetic_states(rng, x, out_len):
    """r_prev [NH, T, 2]: the empty prefix's state for out_len = 0; otherwise per row its own decreasing log-probabilities from
    row out_len - 1 on, LOGZERO before (a prefix of out_len labels cannot end earlier)."""
    T = x.shape[0]
    if out_len == 0:
        return np.repeat(prefix_initial(x, BLANK, np.float32)[None], NH, 0)
    r = np.full((NH, T, 2), LOGZERO, dtype=np.float32)
    first = out_len - 1
    n = T - first
    for h in range(NH):
        for k in range(2):
            r[h, first:, k] = -rng.uniform(0.5, 5.0) - np.cumsum(rng.uniform(0.2, 3.0, n))
    return r


def candidates(rng, nc, last):
    """cs [NH, nc] distinct labels per row; with nc < V: row 0 holds its repeated label, row 1 eos, row 2 blank, row 3 all three,
    at different positions."""
    cs = np.stack([rng.permutation(V)[:nc] for _ in range(NH)])
    if nc < V:
        plants = {0: [int(last[0])], 1: [EOS], 2: [BLANK], 3: [BLANK, int(last[3]), EOS]}
        for h, toks in plants.items():
            row = [c for c in cs[h] if c not in toks][:nc - len(toks)]
            pos = rng.choice(nc, len(toks), replace=False)
            for p, t in zip(sorted(pos), toks):
                row.insert(p, t)
            cs[h] = row
    return cs


@pytest.mark.parametrize("nc", [7, 83])
@pytest.mark.parametrize("T", [499, 1750])
def test_ctc_prefix_scorer_recipe_shapes(cuda, T, nc):
    """CTCPrefixScorer.initial_state and .score (10 hypotheses, each with its own state and last label) against the fp64
    restatement at out_len = 0, 1, 2, T/2, T - 1, T; states compared from row start - 1 = max(out_len, 1) - 1 on."""
    rng = np.random.RandomState(T + nc)
    x = torch.log_softmax(torch.tensor(rng.randn(T, V) * 2.0, dtype=torch.float32), -1)
    xn = x.numpy()
    sc = CTCPrefixScorer(x.to(cuda), BLANK, EOS)
    with poisoned_allocations():
        r0 = sc.initial_state()
    check_log_space(f"initial T{T}", r0.cpu().numpy(), prefix_initial(xn, BLANK), prefix_initial(xn, BLANK, np.float32))
    ratios = []
    for out_len in (0, 1, 2, T // 2, T - 1, T):
        r_prev = synthetic_states(rng, xn, out_len)
        last = rng.choice([c for c in range(V) if c not in (BLANK, EOS)], NH)
        cs = candidates(rng, nc, last)
        with poisoned_allocations():
            psi, r = sc.score(torch.tensor(last, device=cuda), out_len, torch.tensor(cs, device=cuda), torch.tensor(r_prev, device=cuda))
        torch.cuda.synchronize()
        psi, r = psi.cpu().numpy(), r.cpu().numpy()
        assert np.isfinite(r).all(), out_len   # rows before start - 1 are written too (LOGZERO)
        p64, s64 = prefix_score(xn, last, out_len, cs, r_prev, BLANK, EOS, np.float64)
        p32, s32 = prefix_score(xn, last, out_len, cs, r_prev, BLANK, EOS, np.float32)
        s = max(out_len, 1) - 1
        ratios.append(check_log_space(f"log_psi out_len {out_len}", psi, p64, p32))
        ratios.append(check_log_space(f"states out_len {out_len}", r[:, :, s:], s64[:, :, s:], s32[:, :, s:]))
        assert (psi[cs == BLANK] == np.float32(LOGZERO)).all()
    print(f"prefix T{T} nc{nc}: worst kernel / numpy-fp32 error {max(ratios):.3g}")
