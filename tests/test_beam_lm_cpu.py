"""tests/beam_lm_reference.py (the fp64 restatement of st5_beam_lm_logprobs) against torch's own expression in fp64:
torch.log_softmax(logits / T), lp[:, :V_lm] += w * torch.log_softmax(x_lm); the in-place form after a hand-made CTC mix."""
import pytest
import torch

from tests import beam_lm_reference as R

TOL = 1e-12      # fp64 against fp64: two orders of the same few operations on values below 100


def _case(rows, V, V_lm, seed, lm_dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, V + 3, generator=g) * 3          # (a row stride: columns past V are never read)
    logits[:, V:] = 1e9
    lm = (torch.randn(rows, V_lm, generator=g) * 4).to(lm_dtype)
    return logits, lm


@pytest.mark.parametrize("lm_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("T", [1.0, 0.25])
@pytest.mark.parametrize("rows,V,V_lm", [(1, 36, 36), (7, 36, 34), (7, 83, 83), (5, 1000, 998)])
def test_logits_form_is_torchs_expression(rows, V, V_lm, T, lm_dtype):
    logits, lm = _case(rows, V, V_lm, seed=V + rows, lm_dtype=lm_dtype)
    logits[0, 5] = float("-inf")
    w = 0.3
    want = torch.log_softmax(logits[:, :V].double() / T, -1)
    want[:, :V_lm] += w * torch.log_softmax(lm.double(), -1)
    got = R.fuse_logits(logits, V, T, lm, w)
    assert got.dtype == torch.float64 and got.shape == (rows, V)
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and float(got[0, 5]) == float("-inf")
    fin = torch.isfinite(want)
    assert (got[fin] - want[fin]).abs().max().item() <= TOL
    if V_lm < V:                                                # no LM term past V_lm
        plain = torch.log_softmax(logits[:, :V].double() / T, -1)
        assert (got[:, V_lm:] - plain[:, V_lm:]).abs().max().item() <= TOL


def test_weight_zero_and_nan_rows():
    logits, lm = _case(4, 36, 34, seed=3)
    plain = R.log_probs(logits[:, :36], 1.0)
    assert torch.equal(R.fuse_logits(logits, 36, 1.0, lm, 0.0), plain)
    logits[2, 7] = float("nan")
    got = R.fuse_logits(logits, 36, 1.0, lm, 0.3)
    assert torch.isnan(got[2]).all() and torch.isfinite(got[[0, 1, 3]]).all()


def test_in_place_form_after_a_ctc_mix():
    """What _generate does: CTC mix on the candidates of the unfused log-probabilities, then the LM term on the first V_lm columns."""
    rows, V, V_lm, nc, w_ctc, w = 6, 36, 34, 9, 0.4, 0.3
    logits, lm = _case(rows, V, V_lm, seed=9)
    g = torch.Generator().manual_seed(10)
    lp = torch.log_softmax(logits[:, :V], -1)                   # fp32, as the step holds it
    cs = torch.topk(lp, nc, dim=-1)[1]
    log_psi = -torch.rand(rows, nc, generator=g) * 5
    log_psi[1, 2] = float("-inf")                               # an impossible extension
    mixed = (1 - w_ctc) * lp.gather(1, cs) + w_ctc * log_psi
    lp = lp.scatter(1, cs, mixed)
    wide = torch.full((rows, V + 2), 7.0)
    wide[:, :V] = lp
    want = lp.double().clone()
    want[:, :V_lm] += w * torch.log_softmax(lm.double(), -1)
    got = R.fuse_in_place(wide, V, lm, w)
    assert got.shape == (rows, V) and float(got[1, cs[1, 2]]) == float("-inf")
    fin = torch.isfinite(want)
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and (got[fin] - want[fin]).abs().max().item() <= TOL
    assert torch.equal(got[:, V_lm:], lp[:, V_lm:].double())
    assert (wide[:, V:] == 7.0).all() and torch.equal(wide[:, :V], lp), "the input is left alone"
