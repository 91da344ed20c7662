"""st5_beam_step_sents / st5_beam_reorder_sents / st5_beam_embed_sents / st5_beam_sents_admit (csrc/beam_step.hip) alone, compared by
bytes against the existing scalar kernels and against the numpy restatement of tests/beam_stream_reference.py.

3 slots; beam in 1, 2, 5, 32; V in 2 * beam + 1, 83, 10007; Tmax 6 to 8.
1. all pos equal, no slot done: the per-sentence step writes the bytes st5_beam_step writes at that counter (tok, score, parent, ignore
   flags, records, the ruled log-probabilities), step after step up to the limit;
2. a scripted stream with staged admissions, so that one launch sees pos = (0, min_len - 1, maxlen): after every tick each slot equals
   a single-sentence launch of the existing kernel at its own step, and the whole state equals the restatement; a slot done by its
   limit and a slot done by `beam` hypotheses then wait: every byte of their state and records stays, moved is 0, their log-probability
   rows are never written, and the reorder moves exactly the moved slots; a dirty slot handed to a new sentence runs like a fresh one;
3. admit: the slot's state is a fresh BeamStepState's, its padding bytes are right, every neighbour's bytes are unchanged, a slot index
   outside the stream admits nothing;
4. the pre-net row at mixed positions is st5_beam_embed_step's at each slot's own counter."""
import numpy as np
import pytest
import torch

from tests.beam_stream_reference import BeamStreamRef

pytestmark = pytest.mark.gpu

PAD, EOS, UNK = 1, 2, 3
N_SLOTS, S_ENC = 3, 5
SHAPES = [(beam, V, 4 + (i + j) % 3) for i, beam in enumerate((1, 2, 5, 32)) for j, V in enumerate((2 * beam + 1, 83, 10007))]   # cap: Tmax 6 .. 8
MIN_LEN = 3


def _never(V):
    never = np.zeros(V, bool)
    if V > 5:
        never[[4, V - 1]] = True
    return never


def _rules(cuda, V, cap, min_len):
    from speecht5_amd import functional as Fn
    kw = dict(temperature=1.0, pad=PAD, unk=UNK, eos=EOS, unk_penalty=0.5, min_len=min_len)
    return dict(never=torch.from_numpy(_never(V).astype(np.uint8)).to(cuda), len_div=Fn.beam_len_div(cap, 1.3, cuda), kw=kw)


def _ref(beam, V, cap, min_len):
    return BeamStreamRef(N_SLOTS, beam, V, cap, S=S_ENC, pad=PAD, unk=UNK, eos=EOS, unk_penalty=0.5, min_len=min_len, normalize_scores=True,
                         len_penalty=1.3, never=_never(V))


def _admit(st, ref, kpm, entries):
    from speecht5_amd import functional as Fn
    desc = torch.tensor(entries, dtype=torch.int32, device=st.tok.device).view(-1, 4)
    Fn.beam_sents_admit(desc, len(entries), st, kpm)
    if ref is not None:
        for e in entries:
            ref.admit(*e)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _g(t):
    return t.cpu().numpy()


def _logits(g, rows, V, cuda):
    x = torch.randn(rows, V, generator=g) * 3
    x[:, EOS] -= 40.0                                   # no eos unless a tick asks for it
    return x.to(cuda)


def _tick(st, ref, rules, logits):
    """One per-sentence step and reorder on the kernels, the same on the restatement fed with the kernel's ruled log-probabilities."""
    from speecht5_amd import functional as Fn
    rows, V = logits.shape
    wide = torch.full((rows, V + 3), 1e9, device=logits.device)        # (a row stride: columns past V must never be read)
    wide[:, :V] = logits
    lp = torch.full((rows, V), 7.0, device=logits.device)
    Fn.beam_step_sents(wide, V, st, rules["never"], rules["len_div"], lprobs=lp, **rules["kw"])
    Fn.beam_reorder_sents(st)
    torch.cuda.synchronize()
    if ref is not None:
        live = [ref.live(s) for s in range(ref.n_slots)]
        ref.step(lp.cpu().numpy(), ruled=True)
        ref.reorder()
        for s, on in enumerate(live):
            if not on:
                assert (lp[s * ref.beam:(s + 1) * ref.beam] == 7.0).all(), "a done slot's log-probabilities are never written"
    return lp


def _assert_same(st, ref, what):
    f = ref.full
    assert np.array_equal(_g(st.pos), ref.pos) and np.array_equal(_g(st.maxlen), ref.maxlen), f"{what}: pos / maxlen"
    assert np.array_equal(_g(st.done), ref.done) and np.array_equal(_g(st.moved), ref.moved), f"{what}: done / moved"
    assert np.array_equal(_g(st.pos_rows), ref.pos_rows), f"{what}: pos_rows"
    assert np.array_equal(_g(st.tok), f.tok), f"{what}: tokens"
    assert np.array_equal(_bits(_g(st.score)), _bits(f.score)), f"{what}: cumulative scores (bits)"
    assert np.array_equal(_g(st.parent), f.parent), f"{what}: parents"
    assert np.array_equal(_g(st.ignore).astype(bool), f.ignore), f"{what}: ignore flags"
    assert np.array_equal(_g(st.anc), f.anc), f"{what}: ancestry after the reorder"
    assert np.array_equal(_g(st.n_hyp), f.n_hyp) and np.array_equal(_g(st.rec_len), f.rec_len), f"{what}: record header"
    assert np.array_equal(_g(st.rec_tok), f.rec_tok), f"{what}: record tokens"
    assert np.array_equal(_bits(_g(st.rec_pos)), _bits(f.rec_pos)), f"{what}: positional scores (bits)"
    assert np.array_equal(_bits(_g(st.rec_score)), _bits(f.rec_score)), f"{what}: scores (bits)"


def _slot_bytes(st, s):
    b0, b1 = s * st.beam, (s + 1) * st.beam
    parts = [t[b0:b1] for t in (st.tok, st.score, st.anc, st.ignore, st.parent, st.rec_tok, st.rec_pos, st.rec_score, st.rec_len, st.pos_rows)]
    parts += [t[s:s + 1] for t in (st.pos, st.maxlen, st.done, st.n_hyp)]
    return b"".join(_g(t.contiguous()).tobytes() for t in parts)


@pytest.mark.parametrize("beam,V,cap", SHAPES)
def test_equal_positions_write_the_scalar_kernels_bytes(cuda, beam, V, cap):
    from speecht5_amd import functional as Fn
    min_len = cap                                        # eos is ruled out below the limit: no slot is done before it
    rules = _rules(cuda, V, cap, min_len)
    st = Fn.BeamStreamState(N_SLOTS, beam, cap, cuda)
    sc = Fn.BeamStepState(N_SLOTS, beam, cap, EOS, cuda)
    kpm = torch.zeros(N_SLOTS, S_ENC, dtype=torch.uint8, device=cuda)
    _admit(st, None, kpm, [(s, cap, S_ENC, EOS) for s in range(N_SLOTS)])
    rows = N_SLOTS * beam
    g = torch.Generator().manual_seed(100 * V + beam)
    for step in range(cap + 1):
        logits = _logits(g, rows, V, cuda)
        assert st.pos.tolist() == [step] * N_SLOTS and st.done.tolist() == [0] * N_SLOTS
        lp = _tick(st, None, rules, logits)
        lp2 = torch.full((rows, V), 7.0, device=cuda)
        Fn.beam_step(logits, V, sc, rules["never"], rules["len_div"], lprobs=lp2, **rules["kw"])
        Fn.beam_reorder_dev(sc)
        torch.cuda.synchronize()
        what = f"beam={beam} V={V} cap={cap} step={step}"
        assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32)), f"{what}: ruled log-probabilities"
        for a, b, name in ((st.tok, sc.tok, "tok"), (st.score, sc.score, "score"), (st.parent, sc.parent, "parent"), (st.ignore, sc.ignore, "ignore"),
                           (st.anc, sc.anc, "anc"), (st.rec_tok, sc.rec_tok, "rec_tok"), (st.rec_pos, sc.rec_pos, "rec_pos"),
                           (st.rec_score, sc.rec_score, "rec_score"), (st.rec_len, sc.rec_len, "rec_len"), (st.n_hyp, sc.n_hyp, "n_hyp"),
                           (st.done, sc.sent_done, "done")):
            assert _g(a.contiguous()).tobytes() == _g(b.contiguous()).tobytes(), f"{what}: {name}"
        assert st.moved.tolist() == [1] * N_SLOTS and st.pos_rows.tolist() == [step + 1] * rows
    assert st.done.tolist() == [1] * N_SLOTS and int(sc.n_finished) == N_SLOTS and int(st.n_hyp.min()) >= 1


class _Single:
    """One sentence on the EXISTING kernels (st5_beam_step / st5_beam_reorder_dev), stepped beside a slot of the stream."""

    def __init__(self, cuda, beam, max_len):
        from speecht5_amd import functional as Fn
        self.st = Fn.BeamStepState(1, beam, max_len, EOS, cuda)

    def tick(self, logits, rules, cap):
        from speecht5_amd import functional as Fn
        V = logits.shape[1]
        self.lp = torch.full(tuple(logits.shape), 7.0, device=logits.device)
        len_div = rules["len_div"][:self.st.max_len + 1].contiguous()
        Fn.beam_step(logits.contiguous(), V, self.st, rules["never"], len_div, lprobs=self.lp, **rules["kw"])
        Fn.beam_reorder_dev(self.st)

    def assert_slot(self, st, s, lp, what):
        sc, beam = self.st, st.beam
        b0, b1 = s * beam, (s + 1) * beam
        counter = int(sc.counter)
        assert int(st.pos[s]) == counter and int(st.done[s]) == int(sc.sent_done[0]), f"{what}: position / done"
        n = min(counter, sc.max_len) + 1
        assert torch.equal(st.tok[b0:b1, :n], sc.tok[:, :n]), f"{what}: tokens"
        assert torch.equal(st.score[b0:b1, :n].view(torch.int32), sc.score[:, :n].view(torch.int32)), f"{what}: scores (bits)"
        assert torch.equal(st.anc[b0:b1, :n] - b0, sc.anc[:, :n]), f"{what}: ancestry"
        if 1 <= counter <= sc.max_len:
            assert torch.equal(st.parent[b0:b1] - b0, sc.parent), f"{what}: parents"
        assert torch.equal(st.ignore[b0:b1], sc.ignore), f"{what}: ignore flags"
        assert torch.equal(lp[b0:b1].view(torch.int32), self.lp.view(torch.int32)), f"{what}: ruled log-probabilities"
        nh = int(sc.n_hyp[0])
        assert int(st.n_hyp[s]) == nh, f"{what}: hypothesis count"
        for k in range(nh):
            L = int(sc.rec_len[k])
            assert int(st.rec_len[b0 + k]) == L and torch.equal(st.rec_tok[b0 + k, :L], sc.rec_tok[k, :L]), f"{what}: record {k}"
            assert torch.equal(st.rec_pos[b0 + k, :L].view(torch.int32), sc.rec_pos[k, :L].view(torch.int32)), f"{what}: record {k} (bits)"
            assert torch.equal(st.rec_score[b0 + k].view(torch.int32), sc.rec_score[k].view(torch.int32)), f"{what}: score {k} (bits)"


@pytest.mark.parametrize("beam,V,cap", SHAPES)
def test_scripted_stream_matches_singles_and_the_restatement(cuda, beam, V, cap):
    from speecht5_amd import functional as Fn
    rules = _rules(cuda, V, cap, MIN_LEN)
    st = Fn.BeamStreamState(N_SLOTS, beam, cap, cuda)
    ref = _ref(beam, V, cap, MIN_LEN)
    kpm = torch.zeros(N_SLOTS, S_ENC, dtype=torch.uint8, device=cuda)
    rows = N_SLOTS * beam
    g = torch.Generator().manual_seed(7 * V + beam)
    limit2 = 4                                           # slot 2's limit: 4 <= cap
    singles = {}
    tick_no = [0]

    def tick(boost_eos=()):
        logits = _logits(g, rows, V, cuda)
        for s in boost_eos:
            logits[s * beam:(s + 1) * beam, EOS] += 100.0
        live = [s for s in range(N_SLOTS) if ref.live(s)]
        before = {s: _slot_bytes(st, s) for s in range(N_SLOTS) if s not in live}
        for s in live:
            singles[s].tick(logits[s * beam:(s + 1) * beam], rules, cap)
        lp = _tick(st, ref, rules, logits)
        what = f"beam={beam} V={V} cap={cap} tick={tick_no[0]}"
        tick_no[0] += 1
        _assert_same(st, ref, what)
        for s in live:
            singles[s].assert_slot(st, s, lp, f"{what} slot {s}")
        for s, b in before.items():
            assert _slot_bytes(st, s) == b and int(st.moved[s]) == 0, f"{what}: done slot {s} must not change"
        for s in live:
            assert int(st.moved[s]) == 1

    def admit(s, max_len, frames):
        _admit(st, ref, kpm, [(s, max_len, frames, EOS)])
        singles[s] = _Single(cuda, beam, max_len)

    admit(2, limit2, 3)
    for _ in range(limit2 - (MIN_LEN - 1)):
        tick()
    admit(1, cap, 5)
    for _ in range(MIN_LEN - 1):
        tick()
    admit(0, cap, 1)
    assert st.pos.tolist() == [0, MIN_LEN - 1, limit2] and st.done.tolist() == [0, 0, 0]
    tick()                                               # pos = (0, min_len - 1, maxlen) in one launch; slot 2 reaches its limit
    assert st.done.tolist() == [0, 0, 1] and int(st.pos[2]) == limit2 + 1 and int(st.n_hyp[2]) >= 1
    tick(boost_eos=(1,))                                 # slot 1 collects `beam` hypotheses below its limit; slot 2 waits
    assert st.done.tolist() == [0, 1, 1] and int(st.n_hyp[1]) == beam and int(st.pos[1]) == MIN_LEN + 1 <= cap
    anc_before = st.anc.clone()
    tick()                                               # slots 1 and 2 wait; only slot 0's ancestry rows may move
    assert torch.equal(st.anc[beam:], anc_before[beam:]) and st.moved.tolist() == [1, 0, 0]
    admit(2, 2, 4)                                       # a dirty slot handed on: from here it must run like a fresh sentence
    assert st.done.tolist() == [0, 1, 0]
    for _ in range(3):
        tick()
    assert int(st.done[2]) == 1 and int(st.pos[2]) == 3


@pytest.mark.parametrize("beam,V,cap", SHAPES[::3])
def test_admit_resets_one_slot_and_nothing_else(cuda, beam, V, cap):
    from speecht5_amd import functional as Fn
    st = Fn.BeamStreamState(N_SLOTS, beam, cap, cuda)
    kpm = torch.full((N_SLOTS, S_ENC), 9, dtype=torch.uint8, device=cuda)
    g = torch.Generator().manual_seed(beam)
    for t in (st.tok, st.anc, st.parent, st.rec_tok, st.image, st.pos_rows):       # dirt everywhere
        t.copy_(torch.randint(1, 50, tuple(t.shape), generator=g).to(torch.int32))
    st.score.fill_(-3.5)
    st.ignore.fill_(1)
    before = {s: _slot_bytes(st, s) for s in range(N_SLOTS)}
    kpm_before = kpm.clone()
    moved = st.moved.clone()
    _admit(st, None, kpm, [(1, cap + 9, 3, 7), (N_SLOTS, 2, 2, 2), (-1, 2, 2, 2)])   # the limit is clamped; two slots outside the stream
    torch.cuda.synchronize()
    fresh = Fn.BeamStepState(1, beam, cap, 7, cuda)
    b0, b1 = beam, 2 * beam
    assert torch.equal(st.anc[b0:b1] - b0, fresh.anc) and torch.equal(st.tok[b0:b1, 0], fresh.tok[:, 0])
    assert torch.equal(st.score[b0:b1, 0], fresh.score[:, 0]) and torch.equal(st.ignore[b0:b1], fresh.ignore)
    assert int(st.n_hyp[1]) == 0 and st.rec_len[b0:b1].tolist() == [0] * beam
    assert int(st.pos[1]) == 0 and st.pos_rows[b0:b1].tolist() == [0] * beam and int(st.maxlen[1]) == cap and int(st.done[1]) == 0
    assert kpm[1].tolist() == [0, 0, 0, 1, 1]
    for s in (0, 2):
        assert _slot_bytes(st, s) == before[s], f"slot {s} must not change"
        assert torch.equal(kpm[s], kpm_before[s])
    assert torch.equal(st.moved, moved)
    _admit(st, None, kpm, [(0, 1, S_ENC + 4, EOS), (2, 0, -3, EOS)])                  # frames clamped into [0, S]
    assert kpm[0].tolist() == [0] * S_ENC and kpm[2].tolist() == [1] * S_ENC and st.maxlen.tolist() == [1, cap, 0]


def test_embed_row_at_mixed_positions(cuda):
    """Row r's pre-net row is st5_beam_embed_step's at the counter pos[r // beam], bit for bit (a position past the table is clamped)."""
    from speecht5_amd import functional as Fn
    from speecht5_amd.modules.common import SinusoidalPositionalEmbedding
    V, C, beam, cap = 37, 48, 3, 6
    g = torch.Generator().manual_seed(2)
    table = torch.randn(V, C, generator=g).to(cuda)
    st = Fn.BeamStreamState(N_SLOTS, beam, cap, cuda)
    sc = Fn.BeamStepState(N_SLOTS, beam, cap, EOS, cuda)
    st.tok.copy_(torch.randint(4, V, tuple(st.tok.shape), generator=g).to(torch.int32))
    sc.tok.copy_(st.tok)
    pos = SinusoidalPositionalEmbedding(C, PAD).table(cap + 2 + PAD + 2, cuda)
    for dtype in (torch.float32, torch.bfloat16):
        for positions in ([0, 3, cap + 1], [5, 5, 1], [-4, 2, cap + 40]):
            st.pos.copy_(torch.tensor(positions, dtype=torch.int32))
            y = Fn.beam_embed_sents(table, st, pos, PAD + 1, 6.5, torch.empty(N_SLOTS * beam, C, dtype=dtype, device=cuda))
            for s, p in enumerate(positions):
                sc.counter.fill_(p)
                want = Fn.beam_embed_step(table, sc, pos, PAD + 1, 6.5, torch.empty(N_SLOTS * beam, C, dtype=dtype, device=cuda))
                assert torch.equal(y[s * beam:(s + 1) * beam], want[s * beam:(s + 1) * beam]), (dtype, positions, s)
