"""The numpy restatement of the device beam step (tests/beam_step_reference.py) held to three things, on the CPU:
(a) the existing generator: whole searches on the fake model of tests/fake_seq_model.py driven through the restatement WITHOUT
    shrinking the batch return the hypotheses SequenceGenerator returns for the same cases -- tokens identical, scores and positional
    scores bit-equal (one fp32 add per step, one divide).  torch.topk has no tie rule, so every case is asserted to have no exact tie
    among the finite candidates at ranks 1 .. 2 * beam + 1 of any sentence and step (no case is left out);
(b) planted faults: each way of getting the step wrong is caught by the comparison of (a) or by the finished-sentence count;
(c) the tie rule itself: duplicated log-probabilities, rows of all -inf, max_len forcing with fewer than 2 * beam finite candidates."""
import numpy as np
import pytest
import torch

from tests.beam_step_reference import FAULTS, NEG, BeamStepRef
from tests.fake_seq_model import CASES, FakeSeqModel, fake_sample
from tests.util import Task

# the attention-only cases of the fake golden's case list (no prefix, no n-gram blocking), then seeded ones
SEARCHES = {name: (CASES[name]["kw"], 0, 5) for name in ("beam1", "beam4", "beam5_lenpen_unnorm", "beam3_minlen")}
SEARCHES.update(
    beam2_temp=(dict(beam_size=2, max_len_b=10, temperature=1.7), 1, 6),
    beam8_unk=(dict(beam_size=8, max_len_b=9, unk_penalty=0.7, len_penalty=1.3), 2, 7),
    beam3_short=(dict(beam_size=3, max_len_b=3, min_len=2), 3, 8),
    beam6_unnorm=(dict(beam_size=6, max_len_b=12, normalize_scores=False, min_len=3), 4, 9),
)


def never_of(gen):
    never = np.zeros(gen.vocab_size, bool)
    never[gen.blank] = True
    if gen.mask != gen.unk:
        never[gen.mask] = True
    never[gen.mask_idxs.numpy()] = True
    return never


def drive(kw, model_seed, sample_seed, faults=()):
    """One search through the restatement, and the existing generator's result for the same case."""
    from speecht5_amd.sequence_generator import SequenceGenerator
    d = Task().dicts["text"]
    model = FakeSeqModel(len(d), seed=model_seed).eval()
    sample = fake_sample(seed=sample_seed)
    gen = SequenceGenerator([model], d, **kw)
    with torch.no_grad():
        want = gen.generate([model], dict(sample))
        src = sample["net_input"]["source"]
        n_sent, beam = src.size(0), gen.beam_size
        max_len = min(int(gen.max_len_a * src.size(1) + gen.max_len_b), gen.max_len - 1)
        ref = BeamStepRef(n_sent, beam, gen.vocab_size, max_len, gen.eos, pad=gen.pad, unk=gen.unk, eos=gen.eos,
                          unk_penalty=gen.unk_penalty, min_len=gen.min_len, normalize_scores=gen.normalize_scores,
                          len_penalty=gen.len_penalty, never=never_of(gen), faults=faults)
        enc = gen.model.forward_encoder(sample["net_input"])
        enc = gen.model.reorder_encoder_out(enc, torch.arange(n_sent).repeat_interleave(beam))
        while ref.counter <= max_len and ref.n_finished < n_sent:
            t = ref.counter
            toks = np.stack([ref.history(r, t)[0] for r in range(ref.rows)]).astype(np.int64)
            lprobs, _ = gen.model.forward_decoder(torch.from_numpy(toks), enc, [{}], gen.temperature)
            ref.step(lprobs.numpy())
            ref.reorder()
    return ref, want


def same(ref, want):
    got = ref.hypotheses()
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if len(g) != len(w):
            return False
        for a, b in zip(g, w):
            if a["tokens"].tolist() != b["tokens"].tolist():
                return False
            if np.float32(a["score"]).tobytes() != b["score"].numpy().astype(np.float32).tobytes():
                return False
            if a["positional_scores"].tobytes() != b["positional_scores"].numpy().astype(np.float32).tobytes():
                return False
    return True


@pytest.fixture(scope="module")
def searches():
    return {name: drive(*SEARCHES[name]) for name in SEARCHES}


@pytest.mark.parametrize("name", sorted(SEARCHES))
def test_whole_search_equals_the_existing_generator(searches, name):
    ref, want = searches[name]
    assert ref.min_gap > 0, f"{name}: an exact tie among the finite candidates at ranks 1 .. 2 * beam + 1 (pick another seed)"
    assert ref.n_finished == ref.n_sent and ref.sent_done.all()
    got = ref.hypotheses()
    assert len(got) == len(want)
    for si, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (name, si)
        for hi, (a, b) in enumerate(zip(g, w)):
            assert a["tokens"].dtype == np.int64 and a["tokens"].tolist() == b["tokens"].tolist(), (name, si, hi)
            assert np.float32(a["score"]).tobytes() == b["score"].numpy().tobytes(), (name, si, hi, a["score"], float(b["score"]))
            assert a["positional_scores"].tobytes() == b["positional_scores"].numpy().tobytes(), (name, si, hi)


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_caught(searches, fault):
    """Every fault changes the outcome of at least one search (hypotheses or the finished-sentence count)."""
    caught = [c.__name__ for c in (_dup_case, _all_inf_case, _forced_case, _ignored_case) if c(faults=(fault,)) != c()]
    for name in sorted(SEARCHES):
        if caught or fault == "tie_higher_index_first":   # (the searches are tie-free by construction)
            break
        ref, want = drive(*SEARCHES[name], faults=(fault,))
        if not same(ref, want) or ref.n_finished != ref.n_sent:
            caught.append(name)
    assert caught, f"planted fault {fault!r} went unnoticed"


# ---- (c) the tie rule ----
KW = dict(pad=1, unk=3, eos=2)


def _state(ref):
    return (ref.tok.tobytes(), ref.score.tobytes(), ref.parent.tobytes(), ref.ignore.tobytes(), ref.rec_tok.tobytes(),
            ref.rec_pos.tobytes(), ref.rec_score.tobytes(), ref.n_hyp.tobytes(), ref.n_finished)


def _dup_case(faults=()):
    """Duplicated log-probabilities: tokens 5, 9 and 11 share the best value in every row."""
    ref = BeamStepRef(2, 3, 17, 6, 2, min_len=0, faults=faults, **KW)
    lp = np.full((6, 17), -9.0, np.float32)
    lp[:, [5, 9, 11]] = -1.0
    ref.step(lp)
    ref.reorder()
    ref.step(lp)
    return _state(ref)


def _all_inf_case(faults=()):
    ref = BeamStepRef(1, 2, 9, 4, 2, min_len=0, faults=faults, **KW)
    lp = np.full((2, 9), NEG, np.float32)
    lp[0, 4] = -0.5
    ref.step(lp)
    ref.reorder()
    lp[1] = NEG
    lp[0, 6] = -0.5
    ref.step(lp)
    return _state(ref)


def _forced_case(faults=()):
    """max_len forcing: at step == max_len only eos is finite, `beam` finite candidates among the 2 * beam taken."""
    ref = BeamStepRef(1, 3, 11, 1, 2, min_len=0, faults=faults, **KW)
    g = np.random.default_rng(3)
    lp = np.log(g.dirichlet(np.ones(11), 3)).astype(np.float32)
    ref.step(lp)
    ref.reorder()
    ref.step(lp)
    return _state(ref)


def _ignored_case(faults=()):
    """An eos candidate at a rank whose ignore flag is set is no finished hypothesis (the searches above never set the flag)."""
    ref = BeamStepRef(1, 2, 7, 5, 2, min_len=0, faults=faults, **KW)
    lp = np.log(np.random.default_rng(4).dirichlet(np.ones(7), 2)).astype(np.float32)
    lp[:, 2] = -20.0
    ref.step(lp)
    ref.reorder()
    ref.ignore[0] = True
    lp[:, 2] = -0.01                               # eos is now the best candidate of both rows: ranks 0 and 1
    ref.step(lp)
    return _state(ref)


def test_ignored_rank_is_not_finalised():
    assert np.frombuffer(_ignored_case()[7], np.int32).tolist() == [0], "rank 0 holds eos but is ignored: nothing finishes"
    assert np.frombuffer(_ignored_case(faults=("ignored_slot_finalised",))[7], np.int32).tolist() == [1]


def test_tie_rule_duplicates():
    ref = BeamStepRef(2, 3, 17, 6, 2, min_len=0, **KW)
    lp = np.full((6, 17), -9.0, np.float32)
    lp[:, [5, 9, 11]] = -1.0
    ref.step(lp)
    # step 0: beam row 0 only; the three equal best in token order, then the -9 ties in token order (pad is -inf and comes last)
    assert ref.tok[:3, 1].tolist() == [5, 9, 11] and ref.tok[3:, 1].tolist() == [5, 9, 11]
    assert ref.parent.tolist() == [0, 0, 0, 3, 3, 3]
    ref.reorder()
    ref.step(lp)
    # step 1: nine candidates at -2; the lower flat index beam_row * V + token first: row 0's three
    assert ref.tok[:3, 2].tolist() == [5, 9, 11] and ref.parent[:3].tolist() == [0, 0, 0]
    assert (ref.score[:3, 2] == np.float32(-2)).all()


def test_tie_rule_rows_of_minus_inf():
    ref = BeamStepRef(1, 2, 9, 4, 2, min_len=0, **KW)
    lp = np.full((2, 9), NEG, np.float32)
    lp[0, 4] = -0.5
    ref.step(lp)
    # one finite candidate, then the -inf ones by flat index: token 0 (token 1 is pad: also -inf, same rule)
    assert ref.tok[:, 1].tolist() == [4, 0] and ref.score[0, 1] == np.float32(-0.5) and ref.score[1, 1] == NEG
    assert not ref.ignore.any() and ref.n_hyp[0] == 0


def test_tie_rule_under_max_len_forcing():
    ref = BeamStepRef(1, 3, 11, 1, 2, min_len=0, **KW)
    g = np.random.default_rng(3)
    lp = np.log(g.dirichlet(np.ones(11), 3)).astype(np.float32)
    ref.step(lp)
    ref.reorder()
    before = ref.tok.copy()
    ref.step(lp)                                   # step == max_len: 3 finite candidates (eos of every row), 3 of -inf
    assert ref.n_hyp[0] + 0 >= 1 and ref.sent_done[0] == 1 and ref.n_finished == 1
    assert all(ref.rec_tok[h, ref.rec_len[h] - 1] == 2 for h in range(ref.n_hyp[0]))
    assert np.array_equal(ref.tok, before), "nothing continues at step == max_len"
    ref.step(lp)                                   # the counter is past max_len: nothing changes
    assert ref.counter == 2 and ref.n_finished == 1
