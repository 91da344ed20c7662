"""The per-slot forms of the CTC kernels of a beam-search stream (csrc/beam_ctc.hip: st5_beam_ctc_candidates_sents,
st5_ctc_prefix_score_rows_sents, st5_ctc_select_sents, st5_ctc_sents_admit; csrc/beam_step.hip: st5_beam_step_sents_logprobs) alone,
compared BY BYTES with the scalar kernels (st5_beam_ctc_candidates, st5_ctc_prefix_score_rows_dev, st5_beam_step_logprobs,
st5_ctc_select_dev) at the slot's own step.  3 slots with frame counts (37, 5, 1) in S = 37, cap 4; every output buffer is
poison-filled before a launch (in both arms, so that what a kernel leaves alone compares equal too).

1. all slots at one step, none done: steps 0 .. cap and one past it equal the scalar kernels at that counter;
2. staggered slots, pos = (0, 2, maxlen), then one slot done: each slot equals a one-sentence launch of the scalar kernels at its own
   step (the slots are handed over dirty: NaN state, unknown = 1, old prev); a done slot changes no byte of any CTC buffer;
3. select: only moved slots are touched; a counting row continued outside its parent's candidates sets `unknown` of its own slot and
   no other; an ignored row and a row of a slot finished by that step do not;
4. admit: the state is CTCPrefixScorerRows.initial_state() of that posterior alone repeated by beam, prev 0, unknown 0, frames written,
   neighbours unchanged byte for byte, an out-of-range slot admits nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_SLOTS, S, CAP = 3, 37, 4
FRAMES = (37, 5, 1)
SHAPES = [(41, 1, 7), (41, 3, 7), (10007, 3, 70), (10007, 32, 224)]
PAD, EOS, UNK, W = 1, 2, 3, 0.3
RULES = dict(pad=PAD, unk=UNK, eos=EOS, unk_penalty=0.0, min_len=0)
POISON_F, POISON_I = float.fromhex("-0x1.23456p+100"), -77


def _b(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


class Arms:
    """The posterior, the never mask and the per-tick logits of one shape (shared by both arms)."""

    def __init__(self, cuda, V, beam, nc, ticks=CAP + 4, seed=5):
        g = torch.Generator().manual_seed(seed + V + beam)
        self.cuda, self.V, self.beam, self.nc, self.blank = cuda, V, beam, nc, V - 1
        self.x = torch.log_softmax(torch.randn(N_SLOTS, S, V, generator=g) * 3.0, dim=-1).to(cuda)
        self.never = torch.zeros(V, dtype=torch.uint8)
        self.never[self.blank] = 1
        self.never = self.never.to(cuda)
        logits = torch.randn(ticks, N_SLOTS * beam, V, generator=g) * 6.0
        logits[:, :, EOS] = -60.0                       # (no hypothesis ends before its limit: a slot is done at step == maxlen only)
        self.logits = logits.to(cuda)
        self.len_div = None

    def scalar(self, slots, max_len=CAP):
        """The scalar kernels over the sentences `slots` of the posterior: (BeamStepState, BeamCtcState)."""
        from speecht5_amd import functional as Fn
        from speecht5_amd.sequence_generator import CTCPrefixScorerRows
        idx = list(slots)
        bs = Fn.BeamStepState(len(idx), self.beam, max_len, EOS, self.cuda)
        lens = torch.tensor([FRAMES[s] for s in idx], dtype=torch.int32, device=self.cuda)
        ctc = Fn.BeamCtcState(CTCPrefixScorerRows(self.x[idx], lens, self.blank, EOS), bs, self.nc, W)
        return bs, ctc

    def sents(self):
        from speecht5_amd import functional as Fn
        ss = Fn.BeamStreamState(N_SLOTS, self.beam, CAP, self.cuda)
        ctc = Fn.BeamCtcStreamState(ss, S, self.V, self.nc, W, self.blank, EOS, self.cuda)
        ctc.x.copy_(self.x)
        kpm = torch.zeros(N_SLOTS, S, dtype=torch.uint8, device=self.cuda)
        return ss, ctc, kpm

    def admit(self, ss, ctc, kpm, slots, max_len=CAP):
        from speecht5_amd import functional as Fn
        desc = torch.tensor([[s, max_len, FRAMES[s] if 0 <= s < N_SLOTS else 3, EOS] for s in slots], dtype=torch.int32).to(self.cuda)
        Fn.beam_sents_admit(desc, len(slots), ss, kpm)
        Fn.ctc_sents_admit(desc, len(slots), ss, ctc)


def _poison(ctc):
    ctc.lp.fill_(POISON_F)
    ctc.log_psi.fill_(POISON_F)
    ctc.r_new.fill_(POISON_F)
    ctc.cs.fill_(POISON_I)


def _scalar_step(a, bs, ctc, logits):
    from speecht5_amd import functional as Fn
    _poison(ctc)
    Fn.beam_ctc_candidates(logits, a.V, bs, ctc, a.never, 1.0)
    Fn.ctc_prefix_score_rows_dev(bs, ctc)
    Fn.beam_step(ctc.lp, a.V, bs, a.never, a.len_div, logprobs=True, temperature=1.0, **RULES)
    Fn.ctc_select_dev(bs, ctc)
    Fn.beam_reorder_dev(bs)


def _sents_step(a, ss, ctc, logits):
    from speecht5_amd import functional as Fn
    _poison(ctc)
    Fn.beam_ctc_candidates_sents(logits, a.V, ss, ctc, a.never, 1.0)
    Fn.ctc_prefix_score_rows_sents(ss, ctc)
    Fn.beam_step_sents_logprobs(ctc.lp, a.V, ss, a.never, a.len_div, **RULES)
    Fn.ctc_select_sents(ss, ctc)
    Fn.beam_reorder_sents(ss)


def _rows(t, slot, beam):
    return t[slot * beam:(slot + 1) * beam]


def _ctc_bytes(a, ctc, slot, frames, at=None):
    """The compared CTC arrays of one slot's rows (`at`: the slot's index in the arm, default `slot`): cs, lp, log_psi, r_new over the
    live frames, state, prev."""
    at = slot if at is None else at
    return {name: _b(_rows(getattr(ctc, name), at, a.beam)) for name in ("cs", "lp", "log_psi", "state", "prev")} | {
        "r_new": _b(_rows(ctc.r_new, at, a.beam)[:, :frames])}


def _beam_bytes(a, st, slot, at=None):
    at = slot if at is None else at
    row0, sub = slot * a.beam, at * a.beam
    return {"tok": _b(_rows(st.tok, at, a.beam)), "score": _b(_rows(st.score, at, a.beam)), "ignore": _b(_rows(st.ignore, at, a.beam)),
            "parent": _b(_rows(st.parent, at, a.beam) - sub + row0), "anc": _b(_rows(st.anc, at, a.beam) - sub + row0)}


def _assert_equal(got, want, what):
    for name in want:
        assert got[name] == want[name], f"{what}: {name}"


@pytest.mark.parametrize("V,beam,nc", SHAPES)
def test_equal_positions_are_the_scalar_kernels_at_that_counter(cuda, V, beam, nc):
    a = Arms(cuda, V, beam, nc)
    bs, ctc = a.scalar(range(N_SLOTS))
    ss, ctc_s, kpm = a.sents()
    a.admit(ss, ctc_s, kpm, [0, 1, 2])
    for step in range(CAP + 2):                         # steps 0 .. cap and one past it
        _scalar_step(a, bs, ctc, a.logits[step])
        _sents_step(a, ss, ctc_s, a.logits[step])
        torch.cuda.synchronize()
        assert ss.pos.tolist() == [min(step, CAP) + 1] * N_SLOTS and int(bs.counter) == min(step, CAP) + 1
        assert ss.done.tolist() == [int(step >= CAP)] * N_SLOTS
        for s in range(N_SLOTS):
            _assert_equal(_ctc_bytes(a, ctc_s, s, FRAMES[s]), _ctc_bytes(a, ctc, s, FRAMES[s]), f"step {step} slot {s}")
            _assert_equal(_beam_bytes(a, ss, s), _beam_bytes(a, bs, s), f"step {step} slot {s}")
        assert int(ctc_s.unknown.max()) == int(ctc.unknown)


@pytest.mark.parametrize("V,beam,nc", SHAPES)
def test_staggered_slots_equal_one_sentence_launches_and_a_done_slot_is_left_alone(cuda, V, beam, nc):
    a = Arms(cuda, V, beam, nc)
    ss, ctc_s, kpm = a.sents()
    admit_tick = {2: 0, 1: CAP - 2, 0: CAP}             # after tick CAP - 1: pos = (-, 2, maxlen); slot 0 joins at pos 0
    single = {}
    for tick in range(CAP + 2):
        for s, t0 in admit_tick.items():
            if t0 == tick:
                # handed over dirty: what an earlier occupant may leave behind
                _rows(ctc_s.state, s, beam).fill_(float("nan"))
                _rows(ctc_s.prev, s, beam).fill_(5.0)
                ctc_s.unknown[s] = 1
                ctc_s.frames[s] = 11
                a.admit(ss, ctc_s, kpm, [s])
                single[s] = a.scalar([s])
        if tick == CAP:
            torch.cuda.synchronize()
            assert ss.pos.tolist() == [0, 2, CAP] and ss.done.tolist() == [0, 0, 0] and ss.maxlen.tolist() == [CAP] * 3
        before = {s: (_ctc_bytes(a, ctc_s, s, S), int(ctc_s.unknown[s])) for s in range(N_SLOTS) if int(ss.done[s])}
        _sents_step(a, ss, ctc_s, a.logits[tick])
        for s, t0 in admit_tick.items():
            if t0 <= tick:
                sub = torch.zeros_like(a.logits[tick][:beam]).copy_(_rows(a.logits[tick], s, beam))
                _scalar_step(a, *single[s], sub)
        torch.cuda.synchronize()
        for s in range(N_SLOTS):
            if s in before:
                # a done slot: nothing of it was written, the poison included (it was refilled in front of the step)
                after = _ctc_bytes(a, ctc_s, s, S)
                for name in ("state", "prev"):
                    assert after[name] == before[s][0][name], f"tick {tick}: done slot {s} wrote {name}"
                assert _b(_rows(ctc_s.lp, s, beam)) == _b(torch.full_like(_rows(ctc_s.lp, s, beam), POISON_F))
                assert _b(_rows(ctc_s.cs, s, beam)) == _b(torch.full_like(_rows(ctc_s.cs, s, beam), POISON_I))
                assert _b(_rows(ctc_s.log_psi, s, beam)) == _b(torch.full_like(_rows(ctc_s.log_psi, s, beam), POISON_F))
                assert _b(_rows(ctc_s.r_new, s, beam)) == _b(torch.full_like(_rows(ctc_s.r_new, s, beam), POISON_F))
                assert int(ctc_s.unknown[s]) == before[s][1] and int(ss.moved[s]) == 0
            elif admit_tick[s] <= tick:
                bs1, ctc1 = single[s]
                _assert_equal(_ctc_bytes(a, ctc_s, s, FRAMES[s]), _ctc_bytes(a, ctc1, s, FRAMES[s], at=0), f"tick {tick} slot {s}")
                _assert_equal(_beam_bytes(a, ss, s), _beam_bytes(a, bs1, s, at=0), f"tick {tick} slot {s}")
                assert int(ctc_s.unknown[s]) == int(ctc1.unknown) and int(ss.pos[s]) == int(bs1.counter)
    assert ss.done.tolist() == [0, 0, 1] and ss.pos.tolist() == [2, 4, CAP + 1]


@pytest.mark.parametrize("V,beam,nc", SHAPES)
def test_select_touches_moved_slots_only_and_flags_its_own_slot(cuda, V, beam, nc):
    from speecht5_amd import functional as Fn
    a = Arms(cuda, V, beam, nc)
    ss, ctc, kpm = a.sents()
    a.admit(ss, ctc, kpm, [0, 1, 2])
    g = torch.Generator().manual_seed(9)
    rows, t = N_SLOTS * beam, 2
    ctc.r_new.copy_(torch.randn(rows, S, nc, 2, generator=g))
    ctc.log_psi.copy_(torch.randn(rows, nc, generator=g))
    ctc.cs.copy_(torch.stack([torch.randperm(V - 1, generator=g)[:nc] for _ in range(rows)]).to(torch.int32))
    ss.pos.fill_(t)
    ss.moved.copy_(torch.tensor([1, 0, 1], dtype=torch.int32))
    ss.done.copy_(torch.tensor([0, 0, 1], dtype=torch.int32))          # slot 2 was finished by the step in front
    parent = torch.tensor([s * beam + (b + 1) % beam for s in range(N_SLOTS) for b in range(beam)], dtype=torch.int32)
    ss.parent.copy_(parent)
    pick = torch.randint(0, nc, (rows,), generator=g)
    cs = ctc.cs.cpu()
    tok = torch.tensor([int(cs[parent[r], pick[r]]) for r in range(rows)], dtype=torch.int32)
    outside = [s * beam + beam - 1 for s in range(N_SLOTS)]            # the last row of every slot leaves its parent's candidates
    tok[outside] = V - 1
    ss.tok[:, t] = tok.to(cuda)
    ctc.state.fill_(POISON_F)
    ctc.prev.fill_(POISON_F)
    ctc.unknown.zero_()
    Fn.ctc_select_sents(ss, ctc)
    torch.cuda.synchronize()
    assert ctc.unknown.tolist() == [1, 0, 0], "a counting row of slot 0 alone left its candidates"
    state, prev, r_new, log_psi = ctc.state.cpu(), ctc.prev.cpu(), ctc.r_new.cpu(), ctc.log_psi.cpu()
    logzero = torch.full((2,), -10000000000.0)
    for r in range(rows):
        s, p = r // beam, int(parent[r])
        if s == 1:                                                     # unmoved: untouched
            assert _b(state[r]) == _b(torch.full_like(state[r], POISON_F)) and _b(prev[r:r + 1]) == _b(torch.full((1,), POISON_F))
            continue
        slot = 0 if r in outside else int(pick[r])
        assert _b(state[r, :FRAMES[s]]) == _b(r_new[p, :FRAMES[s], slot]), f"row {r}: state"
        assert all(_b(state[r, f]) == _b(logzero) for f in range(FRAMES[s], S)), f"row {r}: behind the frames"
        assert _b(prev[r:r + 1]) == _b(log_psi[p, slot:slot + 1]), f"row {r}: prev"
    # an ignored row does not count; neither does a parent outside the slot when the row is ignored
    ss.ignore[outside[0]] = 1
    ctc.unknown.zero_()
    Fn.ctc_select_sents(ss, ctc)
    torch.cuda.synchronize()
    assert ctc.unknown.tolist() == [0, 0, 0]
    # a parent in another slot is a broken parent: no state, and only the row's own slot hears of it
    ss.ignore.zero_()
    ss.tok[outside[0], t] = int(cs[parent[outside[0]], 0])
    ss.parent[0] = beam                                                # (row 0 of slot 0 names a row of slot 1)
    ctc.unknown.zero_()
    Fn.ctc_select_sents(ss, ctc)
    torch.cuda.synchronize()
    assert ctc.unknown.tolist() == [1, 0, 0] and bool(torch.isnan(ctc.prev[0]))
    assert _b(ctc.state[0]) == _b(logzero.repeat(S, 1))


@pytest.mark.parametrize("V,beam,nc", SHAPES)
def test_admit_resets_one_slot_and_nothing_else(cuda, V, beam, nc):
    from speecht5_amd.sequence_generator import CTCPrefixScorerRows
    a = Arms(cuda, V, beam, nc)
    ss, ctc, kpm = a.sents()
    g = torch.Generator().manual_seed(4)
    ctc.state.copy_(torch.randn(ctc.state.shape, generator=g))
    ctc.prev.copy_(torch.randn(ctc.prev.shape, generator=g))
    ctc.unknown.fill_(1)
    ctc.frames.fill_(9)
    names = ("x", "frames", "state", "r_new", "log_psi", "prev", "cs", "lp", "unknown")
    ctc.r_new.fill_(POISON_F)
    snap = lambda: {n: getattr(ctc, n).clone() for n in names}         # noqa: E731
    before = snap()
    a.admit(ss, ctc, kpm, [-1, N_SLOTS])                               # out of range: nothing is admitted
    torch.cuda.synchronize()
    assert all(_b(getattr(ctc, n)) == _b(before[n]) for n in names)
    for s in (1, 0, 2):
        before = snap()
        a.admit(ss, ctc, kpm, [s])
        torch.cuda.synchronize()
        lens = torch.tensor([FRAMES[s]], dtype=torch.int32, device=cuda)
        want = CTCPrefixScorerRows(a.x[s:s + 1], lens, a.blank, EOS).initial_state().repeat_interleave(beam, dim=0)
        assert _b(_rows(ctc.state, s, beam)) == _b(want), f"slot {s}: state"
        assert _b(_rows(ctc.prev, s, beam)) == _b(torch.zeros(beam)) and int(ctc.unknown[s]) == 0 and int(ctc.frames[s]) == FRAMES[s]
        for n in ("x", "r_new", "log_psi", "cs", "lp"):
            assert _b(getattr(ctc, n)) == _b(before[n]), f"slot {s}: {n} was written"
        for o in range(N_SLOTS):
            if o != s:
                assert _b(_rows(ctc.state, o, beam)) == _b(_rows(before["state"], o, beam)), f"admit {s}: state of slot {o}"
                assert _b(_rows(ctc.prev, o, beam)) == _b(_rows(before["prev"], o, beam)), f"admit {s}: prev of slot {o}"
                assert int(ctc.unknown[o]) == int(before["unknown"][o]) and int(ctc.frames[o]) == int(before["frames"][o])
