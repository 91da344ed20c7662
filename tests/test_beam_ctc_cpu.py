"""tests/beam_ctc_reference.py against torch on the CPU, and its planted faults: each one changes at least one of the arrays that
tests/test_beam_ctc_gpu.py compares with the kernels' (candidates, mixed log-probabilities, state, prev, unknown)."""
import numpy as np
import pytest
import torch

from tests import beam_ctc_reference as R
from tests.ctc_rows_reference import rows_initial, rows_score

BLANK, EOS = 0, 2
S, BEAM, V, TFR, NC, W = 2, 2, 13, 9, 4, 0.3
LENS = (9, 4)


def _scenario(faults=()):
    """One step of a 2 x 2 batch at out_len = 2 with everything a fault can touch: a never-token with a high log-probability, equal
    values across the candidate boundary, non-zero prev, parents that differ from the rows, an ignored row and a row of a finished
    sentence continued outside their parents' candidates."""
    g = torch.Generator().manual_seed(11)
    rows = S * BEAM
    x = torch.log_softmax(torch.randn(S, TFR, V, generator=g) * 2, -1).numpy()
    lp = torch.log_softmax(torch.randn(rows, V, generator=g) * 2, -1).numpy()
    never = np.zeros(V, bool)
    never[[BLANK, V - 1]] = True
    lp[:, V - 1] = -0.01                                     # a never-token that would win
    lp[0, [5, 7, 9, 11]] = -0.5                              # four equal values, two of them inside nc = 4 ...
    lp[0, [3, 4]] = -0.1                                     # ... behind these two
    cs = R.candidates(lp, never, NC, faults)
    sent = np.repeat(np.arange(S), BEAM)
    last = np.array([4, 5, 6, 7])
    r0 = np.repeat(rows_initial(x, LENS, BLANK, np.float32), BEAM, 0)
    _, r1 = rows_score(x, LENS, sent, np.full(rows, EOS), 0, last[:, None], r0, BLANK, EOS, np.float32)
    r_prev = r1[:, 0]                                        # the states of the prefixes <sos> last[r]
    log_psi, r = rows_score(x, LENS, sent, last, 1, cs, r_prev, BLANK, EOS, np.float32)
    r_new = np.ascontiguousarray(np.transpose(r, (0, 2, 1, 3)))                # [rows, Tfr, nc, 2]
    prev = np.array([-1.5, -2.25, -0.75, -3.0], np.float32)
    mixed = R.mix(lp, cs, log_psi, prev, W, faults)
    parent = np.array([1, 0, 3, 3])
    outside = [t for t in range(1, V - 1) if t not in cs[0].tolist() and t not in cs[3].tolist()][0]
    token = np.array([cs[1, 1], outside, cs[3, 0], outside])
    ignore = np.array([0, 1, 0, 0], bool)                    # row 1: ignored and outside its parent's candidates
    sent_done = np.array([0, 1])                             # row 3: its sentence is finished
    state, prev_new, unknown = R.select(parent, token, cs, log_psi, r_new, LENS, BEAM, ignore, sent_done, faults)
    return dict(lp=lp, never=never, cs=cs, log_psi=log_psi, prev=prev, mixed=mixed, state=state, prev_new=prev_new, unknown=unknown,
                r_new=r_new, parent=parent, token=token)


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.int32) if np.asarray(a[k]).dtype == np.float32 else a[k],
                              np.asarray(b[k]).view(np.int32) if np.asarray(b[k]).dtype == np.float32 else b[k])
               for k in ("cs", "mixed", "state", "prev_new", "unknown"))


def test_candidates_equal_topk_on_tie_free_rows():
    g = torch.Generator().manual_seed(3)
    for V_, nc in ((41, 7), (10007, 70), (300, 224)):
        lp = torch.stack([-(torch.randperm(V_, generator=g).float() * 0.01 + 0.005) for _ in range(5)])    # distinct by construction
        assert all(len(set(row.tolist())) == V_ for row in lp), "the rows must be tie-free"
        never = np.zeros(V_, bool)
        never[[0, 9, V_ - 1]] = True
        masked = lp.clone()
        masked[:, torch.from_numpy(never)] = float("-inf")
        want = torch.topk(masked, nc, dim=-1)[1].numpy()
        assert np.array_equal(R.candidates(lp.numpy(), never, nc), want)


def test_candidates_tie_rule_and_nan():
    lp = np.full((1, 9), -3.0, np.float32)
    lp[0, 6] = np.nan
    lp[0, 4] = -0.0
    lp[0, 8] = 0.0
    never = np.zeros(9, bool)
    never[1] = True
    assert R.candidates(lp, never, 9).tolist() == [[4, 8, 0, 2, 3, 5, 7, 1, 6]]


@pytest.mark.parametrize("w", [0.3, 0.5, 0.4, 0.7])
def test_mix_equals_the_generators_expression_bit_for_bit(w):
    g = torch.Generator().manual_seed(5)
    rows, V_, nc = 6, 41, 7
    lprobs = torch.log_softmax(torch.randn(rows, V_, generator=g) * 3, -1)
    cs = torch.stack([torch.randperm(V_, generator=g)[:nc] for _ in range(rows)])
    log_psi = -torch.rand(rows, nc, generator=g) * 30
    log_psi[0, 0] = R.LOGZERO
    prev = -torch.rand(rows, generator=g) * 20
    want = lprobs.clone()
    mixed = (1 - w) * want.gather(1, cs) + w * (log_psi - prev.unsqueeze(1))       # sequence_generator.py _generate
    want.scatter_(1, cs, mixed.to(want.dtype))
    got = R.mix(lprobs.numpy(), cs.numpy(), log_psi.numpy(), prev.numpy(), w)
    assert np.array_equal(got.view(np.int32), want.numpy().view(np.int32))


def test_select_and_the_unknown_rule():
    base = _scenario()
    assert base["unknown"] == 0, "an ignored row and a finished sentence outside the candidates leave the flag clear"
    assert np.array_equal(base["state"][0, :LENS[0]], base["r_new"][1, :LENS[0], 1]) and base["prev_new"][0] == base["log_psi"][1, 1]
    assert np.array_equal(base["state"][1, :LENS[0]], base["r_new"][0, :LENS[0], 0]), "not among the candidates: slot 0"
    assert (base["state"][2:, LENS[1]:] == np.float32(R.LOGZERO)).all(), "LOGZERO at and behind the sentence's frames"
    live = R.select(base["parent"], base["token"], base["cs"], base["log_psi"], base["r_new"], LENS, BEAM, np.zeros(4, bool),
                    np.array([0, 1]))
    assert live[2] == 1, "the same row, not ignored, sets the flag"


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_is_caught(fault):
    assert _same(_scenario(), _scenario()), "the scenario is deterministic"
    assert not _same(_scenario(), _scenario((fault,))), fault
