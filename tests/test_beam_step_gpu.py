"""st5_beam_step / st5_beam_reorder_dev / st5_beam_embed_step (csrc/beam_step.hip) alone, against tests/beam_step_reference.py.

Seeded fp32 logits go through the kernel with its ruled-lprobs output on; that output is fed to the numpy restatement; after every
step the WHOLE state must be identical: candidate tokens, parents, ignore flags, records, lengths, counters, and the scores bit for
bit.  One scripted sequence per shape covers step 0, step == min_len - 1 (eos wanted, forbidden), a sentence that finishes in the
middle and keeps running, a middle step with ignored ranks and one finished sentence, step == max_len (forcing: fewer than 2 * beam
finite candidates, the rest ordered by the tie rule) and a counter past max_len (nothing changes).  Then the tie cases of
tests/test_beam_step_cpu.py, and the log-softmax against fp64 next to torch.log_softmax on the same logits."""
import os

import numpy as np
import pytest
import torch

from tests.beam_step_reference import BeamStepRef

pytestmark = pytest.mark.gpu

PAD, EOS, UNK = 1, 2, 3
SHAPES = [(V, beam) for V in (41, 83, 10007) for beam in (1, 2, 10, 32) if V - 1 >= 2 * beam]
MAX_LEN, MIN_LEN = 5, 3


def _report(line):
    print(line)
    path = os.environ.get("ST5_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _never(V):
    never = np.zeros(V, bool)
    never[[4, V - 1]] = True
    return never


def _pair(cuda, n_sent, beam, V, max_len, min_len, unk_penalty=0.5, normalize=True, len_penalty=1.3):
    from speecht5_amd import functional as Fn
    st = Fn.BeamStepState(n_sent, beam, max_len, EOS, cuda)
    ref = BeamStepRef(n_sent, beam, V, max_len, EOS, pad=PAD, unk=UNK, eos=EOS, unk_penalty=unk_penalty, min_len=min_len,
                      normalize_scores=normalize, len_penalty=len_penalty, never=_never(V))
    rules = dict(never=torch.from_numpy(_never(V).astype(np.uint8)).to(cuda),
                 len_div=Fn.beam_len_div(max_len, len_penalty, cuda) if normalize else None,
                 kw=dict(temperature=1.0, pad=PAD, unk=UNK, eos=EOS, unk_penalty=unk_penalty, min_len=min_len))
    return st, ref, rules


def _step(st, ref, rules, logits, ld_extra=3):
    """One kernel step and one reference step on the kernel's own ruled log-probabilities; returns those."""
    from speecht5_amd import functional as Fn
    rows, V = logits.shape
    wide = torch.full((rows, V + ld_extra), 1e9, device=logits.device)      # (a row stride: columns past V must never be read)
    wide[:, :V] = logits
    lp = torch.full((rows, V), 7.0, device=logits.device)
    Fn.beam_step(wide, V, st, rules["never"], rules["len_div"], lprobs=lp, **rules["kw"])
    Fn.beam_reorder_dev(st)
    torch.cuda.synchronize()
    past = ref.counter > ref.max_len
    ref.step(lp.cpu().numpy(), ruled=True)
    ref.reorder()
    if past:
        assert (lp == 7.0).all(), "a counter past max_len must write nothing"
    return lp


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _assert_same(st, ref, what):
    g = lambda t: t.cpu().numpy()     # noqa: E731
    assert int(st.counter) == ref.counter and int(st.ticket) == 0, what
    assert np.array_equal(g(st.tok), ref.tok), f"{what}: tokens"
    assert np.array_equal(_bits(g(st.score)), _bits(ref.score)), f"{what}: cumulative scores (bits)"
    assert np.array_equal(g(st.parent), ref.parent), f"{what}: parents"
    assert np.array_equal(g(st.ignore).astype(bool), ref.ignore), f"{what}: ignore flags"
    assert np.array_equal(g(st.anc), ref.anc), f"{what}: ancestry after the reorder"
    assert np.array_equal(g(st.n_hyp), ref.n_hyp) and np.array_equal(g(st.sent_done), ref.sent_done), f"{what}: hypothesis counts"
    assert int(st.n_finished) == ref.n_finished, f"{what}: finished sentences"
    assert np.array_equal(g(st.rec_len), ref.rec_len), f"{what}: record lengths"
    assert np.array_equal(g(st.rec_tok), ref.rec_tok), f"{what}: record tokens"
    assert np.array_equal(_bits(g(st.rec_pos)), _bits(ref.rec_pos)), f"{what}: positional scores (bits)"
    assert np.array_equal(_bits(g(st.rec_score)), _bits(ref.rec_score)), f"{what}: scores (bits)"


@pytest.mark.parametrize("n_sent", [1, 3])
@pytest.mark.parametrize("V,beam", SHAPES)
def test_scripted_sequence_matches_the_reference(cuda, V, beam, n_sent):
    st, ref, rules = _pair(cuda, n_sent, beam, V, MAX_LEN, MIN_LEN)
    rows = n_sent * beam
    g = torch.Generator().manual_seed(1000 * V + 10 * beam + n_sent)
    last = n_sent - 1
    for step in range(MAX_LEN + 2):
        logits = (torch.randn(rows, V, generator=g) * 3).to(cuda)
        if step == MIN_LEN - 1:
            logits[:, EOS] += 30.0                                    # eos wanted everywhere, forbidden below min_len
        if step == 3:
            logits[:beam, EOS] += 60.0                                # sentence 0 collects `beam` hypotheses and stays in the batch
        if step == 4:                                                 # ignored ranks, sentence 0 finished, one more eos candidate
            for t, r in ((st.ignore, ref.ignore),):
                idx = [s * beam + k for s in range(n_sent) for k in {0, beam - 1}]
                t[idx] = 1
                r[idx] = True
            logits[last * beam: last * beam + 2, EOS] += 30.0
        before = None
        if step == MAX_LEN + 1:
            before = [t.clone() for t in (st.tok, st.score, st.parent, st.ignore, st.anc, st.records, st.n_finished, st.counter)]
        lp = _step(st, ref, rules, logits)
        _assert_same(st, ref, f"V={V} beam={beam} n_sent={n_sent} step={step}")
        if step == MIN_LEN - 1:
            assert (lp[:, EOS] == float("-inf")).all() and int(st.n_finished) == 0
        if step == 3:
            assert int(st.sent_done[0]) == 1 and int(st.n_hyp[0]) == beam
        if step == MAX_LEN:
            assert int(st.n_finished) == n_sent and torch.isinf(lp[:, :EOS]).all() and torch.isinf(lp[:, EOS + 1:]).all()
        if before is not None:
            after = (st.tok, st.score, st.parent, st.ignore, st.anc, st.records, st.n_finished, st.counter)
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(after, before)), "past max_len: nothing changes"
    assert int(st.counter) == MAX_LEN + 1


def test_ruled_lprobs_are_the_rules_on_log_softmax(cuda):
    """The kernel's lprobs output = the reference's rules applied to torch's log_softmax(logits / temperature): the same -inf pattern,
    values to round-off (the bit-level statement is the fp64 comparison below)."""
    from speecht5_amd import functional as Fn
    V, beam, n_sent = 83, 2, 3
    st, ref, rules = _pair(cuda, n_sent, beam, V, MAX_LEN, MIN_LEN)
    rules["kw"]["temperature"] = 1.7
    logits = (torch.randn(n_sent * beam, V, generator=torch.Generator().manual_seed(5)) * 3).to(cuda)
    logits[1, 9] = float("nan")
    lp = torch.empty(n_sent * beam, V, device=cuda)
    Fn.beam_step(logits, V, st, rules["never"], rules["len_div"], lprobs=lp, **rules["kw"])
    torch.cuda.synchronize()
    want = torch.log_softmax(logits.cpu() / 1.7, -1).numpy()
    want[1] = np.nan                                                  # (a NaN logit makes its whole row NaN, then -inf)
    want = ref.rules(want, step=0)
    got = lp.cpu().numpy()
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    assert np.abs(got[fin] - want[fin]).max() < 1e-5


# ---- the tie cases of tests/test_beam_step_cpu.py ----
def test_tie_rule_duplicates(cuda):
    st, ref, rules = _pair(cuda, 2, 3, 17, 6, 0, unk_penalty=0.0)
    logits = torch.full((6, 17), -9.0)
    logits[:, [5, 9, 11]] = -1.0
    for step in range(3):
        _step(st, ref, rules, logits.to(cuda))
        _assert_same(st, ref, f"duplicates step {step}")
    assert st.tok[:3, 1].tolist() == [5, 9, 11] and st.parent[:3].tolist() == [0, 0, 0]


def test_tie_rule_rows_of_minus_inf(cuda):
    st, ref, rules = _pair(cuda, 1, 2, 9, 4, 0)
    logits = torch.full((2, 9), float("-inf"))
    logits[0, 5] = 0.5
    _step(st, ref, rules, logits.to(cuda))
    _assert_same(st, ref, "one finite candidate")
    assert st.tok[:, 1].tolist() == [5, 0]
    logits[0, 6] = 0.5                                                # row 1 stays all -inf: every one of its candidates ties
    _step(st, ref, rules, logits.to(cuda))
    _assert_same(st, ref, "a row of -inf")


def test_all_candidates_minus_inf_large_row(cuda):
    """Every candidate -inf in a row longer than one pass: the order is the flat index alone."""
    st, ref, rules = _pair(cuda, 1, 2, 10007, 3, 0)
    logits = torch.full((2, 10007), float("-inf"), device=cuda)
    _step(st, ref, rules, logits)
    _assert_same(st, ref, "all -inf")
    assert st.tok[:, 1].tolist() == [0, 1]


@pytest.mark.parametrize("V,beam", SHAPES)
def test_log_softmax_against_fp64(cuda, V, beam):
    """Kernel and torch.log_softmax on the same device and logits, both against fp64: the kernel's worst absolute error is at most
    2 x torch's (a different summation order and nothing more)."""
    from speecht5_amd import functional as Fn
    n_sent = 3
    st, _, rules = _pair(cuda, n_sent, beam, V, MAX_LEN, 0, unk_penalty=0.0)
    rules["never"].zero_()
    logits = (torch.randn(n_sent * beam, V, generator=torch.Generator().manual_seed(V + beam)) * 4).to(cuda)
    lp = torch.empty(n_sent * beam, V, device=cuda)
    Fn.beam_step(logits, V, st, rules["never"], rules["len_div"], lprobs=lp, **rules["kw"])
    exact = torch.log_softmax(logits.double(), -1)
    theirs = torch.log_softmax(logits, -1)
    keep = torch.ones(V, dtype=torch.bool, device=cuda)
    keep[PAD] = False                                                 # (the one column the rules still touch)
    e_kernel = float((lp.double() - exact)[:, keep].abs().max())
    e_torch = float((theirs.double() - exact)[:, keep].abs().max())
    _report(f"log_softmax V={V:5d} beam={beam:2d} rows={n_sent * beam:3d}: kernel {e_kernel:.3e}  torch {e_torch:.3e}")
    assert e_kernel <= 2 * e_torch


def test_limits_and_arguments(cuda):
    from speecht5_amd import functional as Fn
    with pytest.raises(ValueError, match="beam_size 33"):
        Fn.beam_step_check(33, 1000)
    with pytest.raises(ValueError, match="V - 1"):
        Fn.beam_step_check(10, 20)
    Fn.beam_step_check(10, 21)
    Fn.beam_step_check(32, 83)


def test_embed_step_is_the_prenet_row(cuda):
    """embed_scale * E[token] + pos[counter + padding_idx + 1] = what TextDecoderPrenet gives for the newest position (bitwise)."""
    from speecht5_amd import functional as Fn
    from speecht5_amd.modules.common import SinusoidalPositionalEmbedding
    V, C, n_sent, beam, max_len = 37, 48, 2, 3, 6
    g = torch.Generator().manual_seed(2)
    table = torch.randn(V, C, generator=g).to(cuda)
    st = Fn.BeamStepState(n_sent, beam, max_len, EOS, cuda)
    st.tok.copy_(torch.randint(4, V, st.tok.shape, generator=g).to(torch.int32))
    pe = SinusoidalPositionalEmbedding(C, PAD)
    pos = pe.table(max_len + 2 + PAD + 2, cuda)
    for t in (0, 3, max_len + 1):
        st.counter.fill_(t)
        y = Fn.beam_embed_step(table, st, pos, PAD + 1, 6.5, torch.empty(n_sent * beam, C, device=cuda))
        pidx = torch.full((n_sent * beam, 1), t + PAD + 1, device=cuda)
        want = Fn.embed_rows(table, st.tok[:, t:t + 1].long(), pos=pos, pidx=pidx, emb_scale=6.5)
        assert torch.equal(y, want.view(n_sent * beam, C).to(y.dtype)), t
