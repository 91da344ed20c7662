"""tests/lm_reference.py (the restatement the LM GPU tests compare against) pinned to the transformer_lm composed from the verbatim
reference layers (tests/golden/tiny_s2t_beam_lm.pt, written by tools/make_golden_lm.py): every layer's output, the logits and the
log-probabilities, on right-padded rows and on a sequence that outgrows the initial position table (1024 + pad + 1 rows)."""
import pytest
import torch

from tests.lm_reference import lm_forward, lm_log_probs, positions
from tests.util import load_golden


@pytest.fixture(scope="module")
def fx():
    return load_golden("tiny_s2t_beam_lm.pt")[1]


def _sd(fx, dtype):
    return {k: v.to(dtype) for k, v in fx["lm"]["state_dict"].items()}


@pytest.mark.parametrize("batch", ["padded", "long"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_lm_reference_matches_reference_layers(fx, batch, dtype):
    b = fx["batches"][batch]
    a, z = b["keep"]
    sl = slice(a, z)
    logits, states = lm_forward(_sd(fx, dtype), b["tokens"], fx["lm"]["args"]["decoder_attention_heads"], fx["lm"]["pad"])
    assert len(states) == len(b["inner_states"]) == fx["lm"]["args"]["decoder_layers"] + 1
    tol = 2e-5 if dtype == torch.float32 else 1e-5     # (fp64 vs the reference's fp32: the reference's own round-off)
    for i, (got, ref) in enumerate(zip(states, b["inner_states"])):
        err = (got[:, sl].float() - ref).abs().max().item()
        assert err <= tol * max(1.0, ref.abs().max().item()), (batch, i, err)
    err = (logits[:, sl].float() - b["logits"]).abs().max().item()
    assert err <= tol * max(1.0, b["logits"].abs().max().item()), (batch, "logits", err)
    err = (lm_log_probs(logits)[:, sl].float() - b["lprobs"]).abs().max().item()
    assert err <= tol * max(1.0, b["lprobs"].abs().max().item()), (batch, "lprobs", err)


def test_fixture_covers_padding_and_table_growth(fx):
    pad = fx["lm"]["pad"]
    p = fx["batches"]["padded"]["tokens"]
    assert p.eq(pad).any() and not p[:, 0].eq(pad).any()
    long = fx["batches"]["long"]
    assert int(positions(long["tokens"], pad).max()) >= 1024 + pad + 1
    a, z = long["keep"]
    assert a + pad < 1024 + pad + 1 <= z + pad      # the stored slice straddles the initial table's end
    assert fx["lm"]["vocab"] < 36


def test_golden_cases_cover_the_issue(fx):
    cases = fx["cases"]
    beams = {c["kw"]["beam_size"] for c in cases.values()}
    weights = {c["kw"]["lm_weight"] for c in cases.values()}
    assert {1, 3, 5} <= beams and {0.3, 1.0} <= weights
    assert any(c["kw"].get("ctc_weight", 0) > 0 for c in cases.values())
    assert any(c["prefix"] is not None for c in cases.values())
    assert any(c["kw"].get("min_len", 1) > 1 for c in cases.values())
    assert any(any(b < a for a, b in zip(c["lm_rows"], c["lm_rows"][1:])) for c in cases.values())   # a batch shrink
