"""Pins the CTC references of tests/ctc_reference.py to brute force: sums over every alignment of a few frames over a vocabulary
of at most 4 symbols (at most 4^6 = 4096 paths).  tests/test_ctc_gpu.py holds csrc/ctc_loss.hip and csrc/ctc_prefix.hip to these
references, so they stand on the definition of CTC rather than on their own reading of it.

- ctc_loss_ref: nll and gradient (torch's convention exp(lp) - posterior, directly and through a log-softmax) with repeated
  labels, an empty target, an impossible target, an input length of 0, zero_infinity on and off.
- prefix_initial / prefix_score: the prefix probability of every candidate (the repeat-after-blank rule, eos, blank) and the
  extended prefixes' states, along a chain of prefixes up to one label short of the frame count."""
import itertools

import numpy as np
import pytest
import torch

from tests.ctc_reference import LOGZERO, ctc_loss_ref, prefix_initial, prefix_score

D64 = torch.float64


def _paths(T, V):
    return np.array(list(itertools.product(range(V), repeat=T)), dtype=np.int64).reshape(-1, T)


def _collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != blank and c != prev:
            out.append(int(c))
        prev = c
    return tuple(out)


def brute_ctc(lp, target, blank):
    """lp [Tb, V] fp64 -> (nll, grad [Tb, V] = exp(lp) - posterior) by summing over all V^Tb alignments."""
    Tb, V = lp.shape
    if Tb == 0:
        return (0.0 if len(target) == 0 else float("inf")), np.zeros((0, V))
    paths = _paths(Tb, V)
    p = np.exp(lp[np.arange(Tb), paths].sum(1))
    ok = np.array([_collapse(q, blank) == tuple(target) for q in paths])
    total = p[ok].sum()
    post = np.zeros((Tb, V))
    for t in range(Tb):
        np.add.at(post[t], paths[ok, t], p[ok])
    if total == 0:
        return float("inf"), None
    return -np.log(total), np.exp(lp) - post / total


# (target, input length) per sentence: repeats (the l'_s != l'_{s-2} rule), exactly as many frames as the repeats need, an empty
# target, one frame too few for the repeats (impossible), input length 0 with and without labels, one frame
SENTENCES = [([0, 0, 1], 6), ([1, 2, 1], 5), ([1, 1], 3), ([], 5), ([2, 2, 2], 4), ([1], 0), ([], 0), ([2], 1)]


@pytest.mark.parametrize("zero_infinity", [True, False], ids=["zi", "nozi"])
@pytest.mark.parametrize("blank", [3, 0])
def test_ctc_loss_ref_matches_brute_force(blank, zero_infinity):
    gen = torch.Generator().manual_seed(7 + blank)
    T, B, V = 6, len(SENTENCES), 4
    labels = [c for c in range(V) if c != blank]
    tgs = [[labels[i] for i in s] for s, _ in SENTENCES]
    in_len = torch.tensor([n for _, n in SENTENCES])
    tg_len = torch.tensor([len(t) for t in tgs])
    flat = torch.tensor([c for t in tgs for c in t], dtype=torch.long)
    logits = torch.randn(T, B, V, generator=gen) * 1.5
    lprobs = torch.log_softmax(logits, -1)
    g = -0.5
    ref = ctc_loss_ref(lprobs, flat, in_len, tg_len, blank, zero_infinity, grad_out=g, logits=logits)
    lp64 = lprobs.double().numpy()
    impossible = []
    for b, (tg, n) in enumerate(zip(tgs, in_len.tolist())):
        nll, grad = brute_ctc(lp64[:n, b], tg, blank)
        if nll == float("inf"):
            impossible.append(b)
            assert float(ref["nll"][b]) == (0.0 if zero_infinity else float("inf")), b
            if zero_infinity:   # zeroed sentence: no gradient at all
                assert torch.equal(ref["grad"][:, b], torch.zeros(T, V, dtype=D64))
            else:               # torch returns NaN there; tests/test_ctc_gpu.py compares no gradient of such a sentence
                assert torch.isnan(ref["grad"][:n, b]).all()
            continue
        assert abs(float(ref["nll"][b]) - nll) <= 1e-12 * max(1.0, nll), (b, float(ref["nll"][b]), nll)
        want = np.zeros((T, V))
        want[:n] = g * grad
        np.testing.assert_allclose(ref["grad"][:, b].numpy(), want, rtol=0, atol=1e-12, err_msg=f"grad sentence {b}")
        # through the fp64 log-softmax backward: the fp32 rows of lprobs sum to 1 only within fp32 round-off
        want -= torch.softmax(logits[:, b].double(), -1).numpy() * want.sum(-1, keepdims=True)
        np.testing.assert_allclose(ref["grad_logits"][:, b].numpy(), want, rtol=0, atol=1e-12, err_msg=f"grad_logits sentence {b}")
    assert impossible == [4, 5]
    assert torch.isfinite(ref["loss"]) == zero_infinity


def _prefix_brute(x, blank, eos):
    """Probabilities over all V^T paths of x [T, V]: returns functions state(g) -> r [T, 2] (log, -inf for 0) and psi(h, c)."""
    T, V = x.shape
    paths = _paths(T, V)
    p = np.exp(x[np.arange(T), paths].sum(1))
    coll = [[_collapse(q[:t + 1], blank) for t in range(T)] for q in paths]

    def log(v):
        with np.errstate(divide="ignore"):
            return np.log(v)

    def state(g):
        g = tuple(g)
        r = np.zeros((T, 2))
        for i, q in enumerate(paths):
            for t in range(T):
                if coll[i][t] == g:
                    r[t, int(q[t] == blank)] += p[i]
        return log(r)

    def psi(h, c):
        h = tuple(h)
        if c == blank:
            return LOGZERO
        if c == eos:
            return log(sum(p[i] for i in range(len(paths)) if coll[i][-1] == h))
        g = h + (c,)
        return log(sum(p[i] for i in range(len(paths)) if coll[i][-1][:len(g)] == g))

    return state, psi


def _same_log(got, want, tol):
    """got (restated, LOGZERO-style) against want (log of a brute-force probability, -inf for 0)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    zero = np.isneginf(want) | (want <= LOGZERO / 2)
    assert (got[zero] <= LOGZERO / 2).all()
    np.testing.assert_allclose(got[~zero], want[~zero], rtol=0, atol=tol)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 2e-5)], ids=["f64", "f32"])
def test_prefix_score_ref_matches_brute_force(dtype, tol):
    rng = np.random.RandomState(5)
    T, V, blank, eos = 6, 4, 3, 0
    # rows normalised in fp64: a sum over the frames after t is 1 only if every row sums to 1
    x = torch.log_softmax(torch.tensor(rng.randn(T, V) * 1.5, dtype=D64), -1).numpy()
    state, psi = _prefix_brute(x, blank, eos)
    r = prefix_initial(x, blank, dtype)
    _same_log(r, state(()), tol)
    h = []
    cs = np.arange(V)[None]                              # every candidate: labels, eos and blank
    for pick in [1, 1, 2, 1, 2]:                         # 1 then 1: the repeat-after-blank rule
        log_psi, r_new = prefix_score(x, [h[-1] if h else eos], len(h), cs, r[None], blank, eos, dtype)
        assert log_psi.dtype == dtype and r_new.dtype == dtype
        start = max(len(h), 1)
        for c in range(V):
            _same_log(log_psi[0, c], psi(h, c), tol)
            if c not in (eos, blank):
                _same_log(r_new[0, c, start - 1:], state(tuple(h) + (c,))[start - 1:], tol)
        assert log_psi[0, blank] == np.asarray(LOGZERO, dtype)
        h.append(pick)
        r = r_new[0, pick]
