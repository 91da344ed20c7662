"""Pins tests/ctc_rows_reference.py, the yardstick of the rows form of the CTC prefix scorer (tests/test_ctc_rows_gpu.py):
sentence by sentence it is the single-posterior reference on the sentence's own frames; on enumerable cases it is the sum over
every alignment (in the style of tests/test_ctc_reference_cpu.py); a prefix longer than its frames has probability zero for every
label and its own ending probability for eos."""
import numpy as np
import pytest
import torch

from tests.ctc_reference import LOGZERO, prefix_initial, prefix_score
from tests.ctc_rows_reference import rows_initial, rows_score
from tests.test_ctc_reference_cpu import _prefix_brute, _same_log


def _ragged(rng, lens, V, dtype=np.float64, scale=1.5):
    Tmax = max(lens)
    x = torch.log_softmax(torch.tensor(rng.randn(len(lens), Tmax, V) * scale, dtype=torch.float64), -1).numpy().astype(dtype)
    for s, n in enumerate(lens):
        x[s, n:] = np.nan                                          # the padding holds nothing a result may depend on
    return x


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_rows_reference_equals_single_posterior_reference(dtype):
    rng = np.random.RandomState(3)
    lens, V, blank, eos, nc = [9, 1, 14, 6], 11, 10, 2, 5
    x = _ragged(rng, lens, V, dtype)
    sent = np.array([2, 0, 3, 1, 1, 3, 0, 2])
    r0 = rows_initial(x, lens, blank, dtype)
    for s, n in enumerate(lens):
        assert np.array_equal(r0[s, :n], prefix_initial(x[s, :n], blank, dtype))
        assert (r0[s, n:] == np.asarray(LOGZERO, dtype)).all()
    r_prev = r0[sent]
    last = np.full(len(sent), eos)
    labels = [c for c in range(V) if c not in (blank, eos)]
    for out_len in range(5):
        cs = np.stack([rng.permutation(labels)[:nc] for _ in sent])
        if out_len == 2:
            cs[:, 0] = last
        if out_len == 3:
            cs[:, 1], cs[:, 2] = eos, blank
        psi, r = rows_score(x, lens, sent, last, out_len, cs, r_prev, blank, eos, dtype)
        assert psi.dtype == dtype and r.dtype == dtype and np.isfinite(psi).all() and np.isfinite(r).all()
        for h, s in enumerate(sent):
            T = lens[s]
            if out_len <= T:
                p1, r1 = prefix_score(x[s, :T], last[h:h + 1], out_len, cs[h:h + 1], r_prev[h:h + 1, :T], blank, eos, dtype)
                assert np.array_equal(psi[h], p1[0]) and np.array_equal(r[h, :, :T], r1[0])
            assert (r[h, :, T:] == np.asarray(LOGZERO, dtype)).all()
        pick = 0 if out_len == 2 else 3
        last = cs[:, pick]
        r_prev = r[np.arange(len(sent)), pick]


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 2e-5)], ids=["f64", "f32"])
def test_rows_reference_matches_brute_force(dtype, tol):
    """Two sentences of 6 and 3 frames over 4 symbols, every candidate, along a chain of prefixes that outgrows the short one."""
    rng = np.random.RandomState(8)
    lens, V, blank, eos = [6, 3], 4, 3, 0
    x = _ragged(rng, lens, V)
    brute = [_prefix_brute(x[s, :n], blank, eos) for s, n in enumerate(lens)]
    sent = np.array([1, 0, 1])
    r_prev = rows_initial(x, lens, blank, dtype)[sent]
    for h, s in enumerate(sent):
        _same_log(r_prev[h, :lens[s]], brute[s][0](()), tol)
    hist = []
    cs = np.tile(np.arange(V), (len(sent), 1))
    for pick in [1, 1, 2, 1, 2]:                                   # 1 then 1: the repeat-after-blank rule
        last = np.full(len(sent), hist[-1] if hist else eos)
        psi, r = rows_score(x, lens, sent, last, len(hist), cs, r_prev, blank, eos, dtype)
        start = max(len(hist), 1)
        for h, s in enumerate(sent):
            state, bpsi = brute[s]
            for c in range(V):
                _same_log(psi[h, c], bpsi(hist, c), tol)
                if c not in (eos, blank) and start - 1 < lens[s]:
                    _same_log(r[h, c, start - 1:lens[s]], state(tuple(hist) + (c,))[start - 1:], tol)
        hist.append(pick)
        r_prev = r[:, pick]


def test_prefix_longer_than_its_frames():
    rng = np.random.RandomState(9)
    lens, V, blank, eos = [2, 5], 5, 4, 0
    x = _ragged(rng, lens, V)
    sent = np.array([0, 1, 0])
    cs = np.tile(np.arange(V), (3, 1))
    r_prev = -rng.uniform(0.5, 4.0, (3, max(lens), 2))
    psi, r = rows_score(x, lens, sent, np.array([1, 1, 2]), 3, cs, r_prev, blank, eos)
    for h in (0, 2):                                               # 3 labels, 2 frames
        ending = np.logaddexp(r_prev[h, 1, 0], r_prev[h, 1, 1])
        assert psi[h, eos] == ending
        assert (np.delete(psi[h], eos) == LOGZERO).all() and (r[h] == LOGZERO).all()
    assert (psi[1, 1:blank] > LOGZERO / 2).all()                   # the long sentence is scored as ever
    # along a real chain the ending probability of an impossible prefix is itself zero, as the sum over alignments says
    state, bpsi = _prefix_brute(x[0, :2], blank, eos)
    rp = rows_initial(x, lens, blank)[[0]]
    hist = []
    for pick in [1, 2, 1, None]:
        last = np.array([hist[-1] if hist else eos])
        psi, r = rows_score(x, lens, np.array([0]), last, len(hist), cs[:1], rp, blank, eos)
        for c in range(V):
            _same_log(psi[0, c], bpsi(hist, c), 1e-10)
        if pick is None:
            break
        hist.append(pick)
        rp = r[:, pick]
    assert len(hist) == 3 and (psi[0] <= LOGZERO / 2).all()
