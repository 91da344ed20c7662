"""st5_beam_lm_logprobs (csrc/beam_lm.hip) alone: the LM term of a device-stepped beam search step.

1. both forms against the fp64 restatement (tests/beam_lm_reference.py) at LPROBS_TOL, the bar tests/test_beam_step_gpu.py holds
   st5_beam_step's lprobs output to.  The bar is absolute, so the inputs keep |lp| below 64: decoder logits 3 * T * randn (3 * randn
   after the division by T, the spread of that file's logits) and LM logits 4 * randn give at V = 5000 log-probabilities down to
   about -30 and -35; the kernel's fp32 roundings (two subtractions of the log-softmax at half an ulp of 32 = 0.95e-6 each, the LM's
   two scaled by w, the product and the final sum at half an ulp of 64 = 1.9e-6) then add up to about 6e-6;
2. a counter outside [0, max_len] writes nothing;
3. bit properties: w = 0 is st5_beam_ctc_candidates' lp, duplicate rows give duplicate bits, and the logits form followed by
   st5_beam_step_logprobs leaves BeamStepState where st5_beam_step on the same logits leaves it (w = 0)."""
from types import SimpleNamespace

import pytest
import torch

from tests import beam_lm_reference as R

pytestmark = pytest.mark.gpu

LPROBS_TOL = 1e-5      # tests/test_beam_step_gpu.py::test_ruled_lprobs_are_the_rules_on_log_softmax
MAX_LEN, EOS = 5, 2
W = 0.3


def _state(cuda, rows, beam=1, counter=0):
    from speecht5_amd import functional as Fn
    st = Fn.BeamStepState(rows // beam, beam, MAX_LEN, EOS, cuda)
    st.counter.fill_(counter)
    return st


def _inputs(cuda, rows, V, V_lm, T, lm_dtype, seed):
    """Decoder logits and LM logits in rows wider than V / V_lm (what lies past them must never be read), with -inf entries and, from
    7 rows on, one row with a NaN decoder logit."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.full((rows, V + 3), 1e9)
    logits[:, :V] = torch.randn(rows, V, generator=g) * 3 * T
    logits[0, 5] = logits[rows - 1, V - 1] = logits[rows // 2, 0] = float("-inf")
    if rows >= 7:
        logits[3, 9] = float("nan")
    lm = torch.full((rows, V_lm + 5), 1e9)
    lm[:, :V_lm] = torch.randn(rows, V_lm, generator=g) * 4
    lm = lm.to(lm_dtype)
    return logits.to(cuda), lm.to(cuda)[:, :V_lm]


def _assert_close(got, want, what):
    got, want = got.double().cpu(), want.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaN pattern"
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and (got[torch.isinf(got)] < 0).all(), f"{what}: -inf pattern"
    fin = torch.isfinite(want)
    err = float((got[fin] - want[fin]).abs().max())
    print(f"{what}: worst |d| {err:.3e} (bar {LPROBS_TOL:.0e})")
    assert err < LPROBS_TOL, (what, err)


@pytest.mark.parametrize("lm_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("T", [1.0, 0.25])
@pytest.mark.parametrize("narrow", [0, 2], ids=["Vlm=V", "Vlm=V-2"])
@pytest.mark.parametrize("V", [36, 83, 1000, 5000])
@pytest.mark.parametrize("rows", [1, 7, 33])
def test_both_forms_against_the_restatement(cuda, rows, V, narrow, T, lm_dtype):
    from speecht5_amd import functional as Fn
    V_lm = V - narrow
    logits, lm = _inputs(cuda, rows, V, V_lm, T, lm_dtype, seed=rows * 10007 + V + narrow)
    assert logits.stride(0) > V and lm.stride(0) > V_lm
    st = _state(cuda, rows, counter=3)
    # the logits form, into rows wider than V
    lp = torch.full((rows, V + 2), 7.0, device=cuda)
    Fn.beam_lm_logprobs(lp, V, st, lm, W, logits=logits, temperature=T)
    torch.cuda.synchronize()
    assert (lp[:, V:] == 7.0).all(), "columns past V must not be written"
    _assert_close(lp[:, :V], R.fuse_logits(logits.cpu(), V, T, lm.cpu(), W), f"logits form rows={rows} V={V} V_lm={V_lm} T={T}")
    if narrow:                                                   # no LM term past V_lm: the plain log-softmax, bit for bit
        plain = torch.full((rows, V + 2), 7.0, device=cuda)
        Fn.beam_lm_logprobs(plain, V, st, lm, 0.0, logits=logits, temperature=T)
        assert torch.equal(lp[:, V_lm:V].view(torch.int32), plain[:, V_lm:V].view(torch.int32))
    # the in-place form on hand-made mixed log-probabilities (a CTC mix moves a few entries of each row, some to -inf)
    g = torch.Generator().manual_seed(V + rows)
    mixed = torch.log_softmax(torch.randn(rows, V, generator=g) * 3, -1)
    mixed[:, 1::7] = 0.6 * mixed[:, 1::7] - 0.4 * torch.rand(rows, len(range(1, V, 7)), generator=g) * 5
    mixed[0, 8] = mixed[rows - 1, 1] = float("-inf")
    buf = torch.full((rows, V + 2), 7.0, device=cuda)
    buf[:, :V] = mixed.to(cuda)
    before = buf.clone()
    Fn.beam_lm_logprobs(buf, V, st, lm, W)
    torch.cuda.synchronize()
    assert torch.equal(buf[:, V_lm:], before[:, V_lm:]), "columns past V_lm must not be touched in place"
    _assert_close(buf[:, :V], R.fuse_in_place(before.cpu(), V, lm.cpu(), W), f"in place rows={rows} V={V} V_lm={V_lm}")


@pytest.mark.parametrize("counter", [-1, MAX_LEN + 1, MAX_LEN + 7])
def test_a_counter_outside_the_steps_writes_nothing(cuda, counter):
    from speecht5_amd import functional as Fn
    rows, V, V_lm = 7, 83, 81
    logits, lm = _inputs(cuda, rows, V, V_lm, 1.0, torch.float32, seed=1)
    st = _state(cuda, rows, counter=counter)
    lp = torch.full((rows, V), 7.0, device=cuda)
    Fn.beam_lm_logprobs(lp, V, st, lm, W, logits=logits)
    Fn.beam_lm_logprobs(lp, V, st, lm, W)
    torch.cuda.synchronize()
    assert (lp == 7.0).all() and int(st.counter) == counter
    st.counter.fill_(MAX_LEN)                                    # (the last step still writes)
    Fn.beam_lm_logprobs(lp, V, st, lm, W, logits=logits)
    assert not (lp == 7.0).any()


@pytest.mark.parametrize("lm_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("T", [1.0, 0.25])
@pytest.mark.parametrize("rows,V", [(1, 36), (7, 83), (33, 1000), (7, 5000)])
def test_weight_zero_is_the_candidates_lp_bit_for_bit(cuda, rows, V, T, lm_dtype):
    from speecht5_amd import functional as Fn
    V_lm = V - 2
    logits, lm = _inputs(cuda, rows, V, V_lm, T, lm_dtype, seed=V + rows)
    st = _state(cuda, rows, counter=1)
    nc = 7
    ctc = SimpleNamespace(lp=torch.empty(rows, V, device=cuda), cs=torch.zeros(rows, nc, dtype=torch.int32, device=cuda), nc=nc, rows=rows,
                          V=V)
    Fn.beam_ctc_candidates(logits, V, st, ctc, torch.zeros(V, dtype=torch.uint8, device=cuda), T)
    lp = torch.empty(rows, V, device=cuda)
    Fn.beam_lm_logprobs(lp, V, st, lm, 0.0, logits=logits, temperature=T)
    torch.cuda.synchronize()
    nan = torch.isnan(ctc.lp)
    assert torch.equal(torch.isnan(lp), nan) and nan.any() == (rows >= 7)
    assert torch.equal(lp.view(torch.int32)[~nan], ctc.lp.view(torch.int32)[~nan])
    # in place: w = 0 leaves the log-probabilities bit for bit
    buf = ctc.lp.clone()
    Fn.beam_lm_logprobs(buf, V, st, lm, 0.0)
    assert torch.equal(buf.view(torch.int32)[~nan], ctc.lp.view(torch.int32)[~nan]) and torch.equal(torch.isnan(buf), nan)


def test_duplicate_rows_give_duplicate_bits(cuda):
    from speecht5_amd import functional as Fn
    rows, V, V_lm = 33, 1000, 998
    logits, lm = _inputs(cuda, rows, V, V_lm, 1.0, torch.bfloat16, seed=4)
    lm = lm.contiguous()
    for dst, src in ((1, 0), (32, 0), (20, 7)):
        logits[dst] = logits[src]
        lm[dst] = lm[src]
    st = _state(cuda, rows)
    lp = torch.empty(rows, V, device=cuda)
    Fn.beam_lm_logprobs(lp, V, st, lm, W, logits=logits)
    bits = lp.view(torch.int32)
    for dst, src in ((1, 0), (32, 0), (20, 7)):
        assert torch.equal(bits[dst], bits[src])
    Fn.beam_lm_logprobs(lp, V, st, lm, W)
    for dst, src in ((1, 0), (32, 0), (20, 7)):
        assert torch.equal(bits[dst], bits[src])
    assert not torch.equal(bits[2], bits[0])


@pytest.mark.parametrize("V,beam,n_sent", [(36, 3, 2), (83, 10, 1), (1000, 5, 3)])
def test_logits_form_then_the_beam_step_on_logprobs_is_the_beam_step(cuda, V, beam, n_sent):
    """w = 0: st5_beam_lm_logprobs + st5_beam_step_logprobs leaves every buffer of BeamStepState as st5_beam_step on the same logits
    does, step after step (tokens, scores, parents, ignore flags, ancestry, records, counters), bit for bit."""
    from speecht5_amd import functional as Fn
    rows, V_lm = n_sent * beam, V - 2
    a, b = (Fn.BeamStepState(n_sent, beam, MAX_LEN, EOS, cuda) for _ in range(2))
    never = torch.zeros(V, dtype=torch.uint8, device=cuda)
    never[[4, V - 1]] = 1
    len_div = Fn.beam_len_div(MAX_LEN, 1.3, cuda)
    rules = dict(temperature=0.5, pad=1, unk=3, eos=EOS, unk_penalty=0.5, min_len=2)
    g = torch.Generator().manual_seed(V + beam)
    lp = torch.empty(rows, V, device=cuda)
    for step in range(MAX_LEN + 2):
        logits = (torch.randn(rows, V, generator=g) * 3).to(cuda)
        if step == 3:
            logits[:beam, EOS] += 60.0                           # sentence 0 finishes and stays in the batch
        lm = (torch.randn(rows, V_lm, generator=g) * 4).to(cuda)
        Fn.beam_step(logits, V, a, never, len_div, **rules)
        Fn.beam_reorder_dev(a)
        Fn.beam_lm_logprobs(lp, V, b, lm, 0.0, logits=logits, temperature=rules["temperature"])
        Fn.beam_step(lp, V, b, never, len_div, logprobs=True, **rules)
        Fn.beam_reorder_dev(b)
        torch.cuda.synchronize()
        for name in ("counter", "tok", "score", "parent", "ignore", "anc", "records", "n_finished", "ticket"):
            x, y = getattr(a, name), getattr(b, name)
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"step {step}: {name}"
    assert int(a.counter) == MAX_LEN + 1 and int(a.n_finished) == n_sent


def test_arguments(cuda):
    from speecht5_amd import hip
    x, y, lp = (torch.zeros(2, 40, device=cuda) for _ in range(3))
    c = torch.full((1,), MAX_LEN + 1, dtype=torch.int32, device=cuda)      # (a counter past the steps: nothing could be written anyway)
    call = lambda V, V_lm, lm_ld, lp_ld: hip.lib().st5_beam_lm_logprobs(x.data_ptr(), 40, 2, V, 1.0, y.data_ptr(), lm_ld, V_lm, 0.3, hip.F32,  # noqa: E731
                                                                      c.data_ptr(), MAX_LEN, lp.data_ptr(), lp_ld, hip.stream())
    assert call(36, 34, 40, 40) == 0
    assert call(36, 37, 40, 40) == 1, "V_lm > V"
    assert call(36, 34, 33, 40) == 1, "an LM row stride below V_lm"
    assert call(36, 34, 40, 35) == 1, "an lp row stride below V"
