"""Batched joint CTC / attention beam search: the rows form of the CTC prefix scorer (csrc/ctc_prefix.hip: st5_ctc_initial_state_rows,
st5_ctc_prefix_score_rows, st5_ctc_select_rows; sequence_generator.CTCPrefixScorerRows) and SequenceGenerator(ctc_rows=True).

1. kernels, bit for bit: log psi and the valid part of every state equal st5_ctc_prefix_score / st5_ctc_initial_state run per
   sentence on the contiguous slice x[s, :T_s] (no tolerance), and the float32 numpy rows reference within rtol 2e-5 / atol 2e-4
   (the bound tests/test_generator_gpu.py uses for this recursion); a prefix longer than its sentence's frames;
2. select against the torch gather / scatter formulation, bit for bit; known = 0 for a token outside the candidate list;
3. NaN behind every row's end (posterior and previous states) changes no output bit;
4. generator: every sentence of a batch returns the hypotheses of the default path run on that sentence alone;
5. the feature matters: without ctc_rows sentence 1 of a batch does NOT get its single-sentence hypothesis;
6. the default path makes the library calls it made before; 7. a sentence that leaves the batch early; 8. bad arguments."""
import numpy as np
import pytest
import torch

from tests import speech_rows_reference as R
from tests.ctc_reference import LOGZERO
from tests.ctc_rows_reference import rows_initial, rows_score
from tests.util import Task, build_tiny, load_golden, to_dev

pytestmark = pytest.mark.gpu

MARGIN = 1e-4          # (tests/test_speech_rows_gpu.py: the distance a decision must keep from its threshold to be compared)
SCORE_TOL = 2e-4       # tests/test_generator_gpu.py
LZ = np.float32(LOGZERO)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. - 3. kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _posteriors(rng, lens, V, cuda, pad="random"):
    Tmax = max(lens)
    x = torch.log_softmax(torch.tensor(rng.randn(len(lens), Tmax, V) * 2.0, dtype=torch.float32), -1)
    for s, n in enumerate(lens):
        noise = torch.tensor(rng.randn(Tmax - n, V), dtype=torch.float32)     # (drawn in either case: the same candidates follow)
        x[s, n:] = float("nan") if pad == "nan" else noise
    return x.to(cuda)


def _candidates(rng, nh, nc, V, blank, eos, last, step):
    labels = np.array([c for c in range(V) if c not in (blank, eos)])
    if nc <= len(labels):
        cs = np.stack([rng.permutation(labels)[:nc] for _ in range(nh)])
    else:                                                          # a small dictionary: candidates repeat
        cs = np.stack([np.concatenate([rng.permutation(labels), rng.choice(labels, nc - len(labels))]) for _ in range(nh)])
    if step == 2:
        cs[:, 0] = last                                            # the label that repeats the prefix's last one
    if step == 3 and nc >= 3:
        cs[:, 1], cs[:, 2] = eos, blank
    if step == 4:
        cs[::2, nc - 1] = eos                                      # eos in some rows only
    return cs


def _pick(step, nc):
    return 0 if step == 2 or nc < 4 else 3


def _chain(cuda, lens, V, nc, sent, seed, pad="random", poison_states=False, steps=6):
    """Steps 0 .. steps-1 of a decode over rows of mixed sentences: the rows entries against the single-posterior entries on
    x[s, :T_s] (bits) and the float32 numpy rows reference (tolerance).  Returns what the rows entries gave, for test 3."""
    from speecht5_amd.sequence_generator import CTCPrefixScorer, CTCPrefixScorerRows
    rng = np.random.RandomState(seed)
    blank, eos = V - 1, 2
    S, Tmax, nh = len(lens), max(lens), len(sent)
    x = _posteriors(rng, lens, V, cuda, pad)
    xn = x.cpu().numpy()
    lens_t = torch.tensor(lens, dtype=torch.int32, device=cuda)
    sent_t = torch.tensor(sent, dtype=torch.int32, device=cuda)
    rows = CTCPrefixScorerRows(x, lens_t, blank, eos)
    singles = [CTCPrefixScorer(x[s, :n].contiguous(), blank, eos) for s, n in enumerate(lens)]
    r0 = rows.initial_state()
    r0n = rows_initial(xn, lens, blank, np.float32)
    for s, n in enumerate(lens):
        assert torch.equal(r0[s, :n], singles[s].initial_state()), f"initial state of sentence {s}"
        assert bool((r0[s, n:] == LOGZERO).all())
    np.testing.assert_allclose(r0.cpu().numpy(), r0n, rtol=1e-6, atol=1e-5)
    state = r0[sent_t.long()].contiguous()                                    # rows form  [nh, Tmax, 2]
    state1 = [singles[s].initial_state() for s in sent]                       # per row, on its sentence's own frames
    state_np = r0n[np.array(sent)]
    last = np.full(nh, eos)
    out = []
    for step in range(steps):
        cs = _candidates(rng, nh, nc, V, blank, eos, last, step)
        cs_t, last_t = torch.tensor(cs, device=cuda), torch.tensor(last, device=cuda)
        r_prev = state.clone()
        if poison_states:
            for h, s in enumerate(sent):
                r_prev[h, lens[s]:] = float("nan")
        psi, st = rows.score(sent_t, last_t, step, cs_t, r_prev)
        torch.cuda.synchronize()
        psi_np, st_np = rows_score(xn, lens, sent, last, step, cs, state_np, blank, eos, np.float32)
        start = max(step, 1)
        new1 = [None] * nh
        for h, s in enumerate(sent):
            T = lens[s]
            if step <= T:
                p1, r1 = singles[s].score(last_t[h:h + 1], step, cs_t[h:h + 1], state1[h][None])
                assert torch.equal(psi[h], p1[0]), f"step {step} row {h} (sentence {s}, {T} frames): log psi bits"
                assert torch.equal(st[h, :T].permute(1, 0, 2), r1[0]), f"step {step} row {h} (sentence {s}, {T} frames): state bits"
                new1[h] = r1[0]
            else:                                                  # more labels than frames: the rule of the rows form
                got = psi[h].cpu().numpy()
                is_eos = cs[h] == eos
                assert (got[~is_eos] == LZ).all() and bool((st[h, :T] == LOGZERO).all()), (step, h)
                rp = state_np[h, T - 1]
                np.testing.assert_allclose(got[is_eos], np.full(int(is_eos.sum()), np.logaddexp(rp[0], rp[1])), rtol=2e-5, atol=2e-4)
                new1[h] = torch.full((nc, T, 2), LOGZERO, dtype=torch.float32, device=cuda)
            lo = min(start - 1, T)
            np.testing.assert_allclose(st[h, lo:T].permute(1, 0, 2).cpu().numpy(), st_np[h, :, lo:T], rtol=2e-5, atol=2e-4)
        np.testing.assert_allclose(psi.cpu().numpy(), psi_np, rtol=2e-5, atol=2e-4)
        assert (psi.cpu().numpy()[cs == blank] == LZ).all()
        pick = _pick(step, nc)
        parent = torch.arange(nh, device=cuda)
        nstate, nprev, known, nsent = rows.select(sent_t, cs_t, psi, st, parent, cs_t[:, pick].contiguous())
        assert bool(known.all()) and torch.equal(nsent, sent_t) and torch.equal(nprev, psi[:, pick])
        for h, s in enumerate(sent):
            assert torch.equal(nstate[h, :lens[s]], new1[h][pick]) and bool((nstate[h, lens[s]:] == LOGZERO).all())
        out.append((psi.clone(), [st[h, :lens[s]].clone() for h, s in enumerate(sent)], nstate.clone()))
        state, state1 = nstate, [new1[h][pick] for h in range(nh)]
        state_np = st_np[:, pick]
        last = cs[:, pick]
    return out


KERNEL_CASES = [
    ("recipe", [23, 1, 37, 30], 83, [2, 0, 3, 1, 1, 3, 0, 2, 2]),
    ("small_v", [9, 37, 1], 19, [1, 2, 0, 0, 1, 2, 1]),
    ("segments", [2500, 1, 2049, 700], 83, [3, 0, 2, 1, 0, 2]),    # longer than one LDS segment of the walk (2048 frames)
]


@pytest.mark.parametrize("nc", [1, 7, 70])
@pytest.mark.parametrize("name,lens,V,sent", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_rows_entries_bit_equal_to_single_posterior_entries(cuda, name, lens, V, sent, nc):
    assert len(lens) >= 3 and 1 in lens and max(lens) in lens
    _chain(cuda, lens, V, nc, sent, seed=len(name) + nc)


def test_padding_is_never_read(cuda):
    """NaN in x behind every sentence's frames and in r_prev behind every row's frames: the same bits as with finite padding."""
    for name, lens, V, sent in KERNEL_CASES[:2]:
        a = _chain(cuda, lens, V, 7, sent, seed=77)
        b = _chain(cuda, lens, V, 7, sent, seed=77, pad="nan", poison_states=True)
        for (pa, sa, na), (pb, sb, nb) in zip(a, b):
            assert torch.equal(pa, pb) and torch.equal(na, nb)
            assert all(torch.equal(u, v) for u, v in zip(sa, sb))
            assert bool(torch.isfinite(pb).all()) and bool(torch.isfinite(nb).all())


def test_select_equals_torch_gather_and_flags_unknown_tokens(cuda):
    from speecht5_amd.sequence_generator import CTCPrefixScorerRows
    rng = np.random.RandomState(4)
    lens, V, nc, blank, eos = [23, 1, 37, 30], 83, 70, 82, 2
    sent = [2, 0, 3, 1, 1, 3, 0, 2]
    nh, Tmax = len(sent), max(lens)
    x = _posteriors(rng, lens, V, cuda)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=cuda)
    sent_t = torch.tensor(sent, dtype=torch.int32, device=cuda)
    rows = CTCPrefixScorerRows(x, lens_t, blank, eos)
    cs = torch.tensor(_candidates(rng, nh, nc, V, blank, eos, np.full(nh, eos), 0), device=cuda)
    psi, st = rows.score(sent_t, torch.full((nh,), eos, device=cuda), 0, cs, rows.initial_state()[sent_t.long()].contiguous())
    # continued hypotheses: shuffled parents, some twice, some never; the last two tokens are in no candidate list
    parent = torch.tensor([5, 0, 0, 7, 3, 3, 2, 6, 1, 4, 5], device=cuda)
    slot_want = torch.tensor(rng.randint(0, nc, parent.numel()), device=cuda)
    token = cs[parent, slot_want].clone()
    token[-2], token[-1] = blank, eos
    assert not bool((cs[parent[-2:]] == token[-2:, None]).any())
    state, prev, known, nsent = rows.select(sent_t, cs, psi, st, parent, token)
    # the formulation of the default path: slot_of scatter, two advanced-index gathers, the clamp
    slot_of = torch.full((nh, V), -1, dtype=torch.long, device=cuda).scatter_(1, cs, torch.arange(nc, device=cuda).expand_as(cs))
    slot = slot_of[parent, token]
    assert known.dtype == torch.bool and known.tolist() == slot.ge(0).tolist() == [True] * 9 + [False] * 2
    slot_c = slot.clamp(min=0)
    assert slot_c[:-2].tolist() == slot_want[:-2].tolist()
    want = st.permute(0, 2, 1, 3)[parent, slot_c]                  # [n, Tmax, 2]
    assert torch.equal(prev, psi[parent, slot_c]) and torch.equal(nsent, sent_t[parent])
    for i, p in enumerate(parent.tolist()):
        T = lens[sent[p]]
        assert torch.equal(state[i, :T], want[i, :T]), i
        assert bool((state[i, T:] == LOGZERO).all()), i


def test_rows_entries_reject_bad_arguments(cuda):
    from speecht5_amd import hip
    L = hip.lib()
    f = torch.zeros(64, dtype=torch.float32, device=cuda)
    i32 = torch.zeros(8, dtype=torch.int32, device=cuda)
    i64 = torch.zeros(8, dtype=torch.int64, device=cuda)
    u8 = torch.zeros(8, dtype=torch.uint8, device=cuda)
    p, q, l, k = f.data_ptr(), i32.data_ptr(), i64.data_ptr(), u8.data_ptr()
    st = hip.stream()
    assert L.st5_ctc_initial_state_rows(0, q, 1, 2, 4, 3, p, st) == 1
    assert L.st5_ctc_initial_state_rows(p, 0, 1, 2, 4, 3, p, st) == 1
    assert L.st5_ctc_initial_state_rows(p, q, 0, 2, 4, 3, p, st) == 1
    assert L.st5_ctc_initial_state_rows(p, q, 1, 2, 4, 4, p, st) == 1                               # blank outside the dictionary
    assert L.st5_ctc_prefix_score_rows(p, q, 0, 1, 2, 4, 3, 2, p, l, 0, l, 1, 1, p, p, st) == 1       # no sentence index
    assert L.st5_ctc_prefix_score_rows(p, q, q, 1, 2, 4, 3, 2, p, l, -1, l, 1, 1, p, p, st) == 1      # out_len < 0
    assert L.st5_ctc_prefix_score_rows(p, q, q, 1, 2, 4, 3, 2, p, l, 0, l, 1, 1025, p, p, st) == 1    # nc > 1024
    assert L.st5_ctc_prefix_score_rows(p, q, q, 1, 2, 4, 3, 4, p, l, 0, l, 1, 1, p, p, st) == 1       # eos outside the dictionary
    assert L.st5_ctc_select_rows(q, q, 1, 2, l, 1, 1, p, p, l, l, 0, p, p, k, q, st) == 1             # nothing to select
    assert L.st5_ctc_select_rows(q, q, 1, 2, l, 1, 1, p, p, 0, l, 1, p, p, k, q, st) == 1             # no parents
    assert L.st5_ctc_select_rows(q, q, 1, 2, l, 1, 1, p, p, l, l, 1, p, p, 0, q, st) == 1             # no known flags
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. - 7. generator
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(cuda):
    from speecht5_amd import functional as Fn
    model, args = build_tiny(cuda, torch.float32)
    model.eval()
    yield model, args, Task().dicts["text"]
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


def _make_recording_search(d, beam, eos):
    from speecht5_amd.sequence_generator import BeamSearch

    class Recording(BeamSearch):
        """fairseq's beam search, which also keeps the smallest gap between adjacent candidates that a decision hangs on: the
        `beam`-th against the next one (which candidates are looked at for </s>), the last continued hypothesis against the
        next candidate (who continues), and every pair inside the first `beam` of which one closes with </s> (the order in
        which hypotheses are collected).  `all_adjacent` keeps the smallest gap between any two finite neighbours, printed only."""

        def __init__(self):
            super().__init__(d)
            self.decision, self.all_adjacent = float("inf"), float("inf")

        def step(self, step, lprobs, scores, prev_output_tokens=None, original_batch_idxs=None):
            out = super().step(step, lprobs, scores, prev_output_tokens, original_batch_idxs)
            sc, tok = out[0].float().cpu(), out[1].cpu()
            for b in range(sc.size(0)):
                s, is_eos = sc[b], tok[b].eq(eos)
                non_eos = (~is_eos).nonzero().view(-1)
                idx = {beam - 1}
                if non_eos.numel() >= beam:
                    idx.add(int(non_eos[beam - 1]))
                idx |= {i for i in range(beam) if bool(is_eos[i]) or (i + 1 < s.numel() and bool(is_eos[i + 1]))}
                for i in range(s.numel() - 1):
                    if torch.isfinite(s[i]) and torch.isfinite(s[i + 1]):
                        g = float(s[i] - s[i + 1])
                        self.all_adjacent = min(self.all_adjacent, g)
                        if i in idx:
                            self.decision = min(self.decision, g)
            return out

    return Recording()


def _single_run(model, d, clip, beam, kw):
    """The default path on one sentence alone.  Returns its hypotheses and the smallest margins of its decisions:
    (candidates of search.step, boundary of the CTC candidate list, returned hypotheses)."""
    from speecht5_amd.sequence_generator import CTC_SCORING_RATIO, SequenceGenerator
    search = _make_recording_search(d, beam, d.eos())
    gen = SequenceGenerator([model], d, beam_size=beam, search_strategy=search, **kw)
    ctc_beam = min(len(d) - gen.mask_idxs.numel(), int(beam * CTC_SCORING_RATIO))
    boundary = [float("inf")]
    inner, calls = gen._never, [0]

    def never(lprobs):
        # the first call of a step sees the decoder's log-probabilities the CTC candidates are the top ctc_beam of
        out = inner(lprobs)
        calls[0] += 1
        if calls[0] % 2 == 1 and ctc_beam < out.size(-1):
            top = out.float().topk(ctc_beam + 1, dim=-1).values
            g = (top[:, ctc_beam - 1] - top[:, ctc_beam])
            g = g[torch.isfinite(g)]
            if g.numel():
                boundary[0] = min(boundary[0], float(g.min()))
        return out

    gen._never = never
    ni = {"source": clip[None, :], "padding_mask": torch.zeros(1, clip.numel(), dtype=torch.bool, device=clip.device)}
    hyps = gen.generate([model], {"net_input": ni})[0]
    between = min([abs(float(a["score"]) - float(b["score"])) for a, b in zip(hyps, hyps[1:])], default=float("inf"))
    return hyps, dict(decision=search.decision, ctc_list=boundary[0], hyps=between, all_adjacent=search.all_adjacent)


def _batched_run(model, d, wav, pad, beam, kw, ctc_rows=True, prefix_tokens=None):
    from speecht5_amd.sequence_generator import SequenceGenerator
    gen = SequenceGenerator([model], d, beam_size=beam, exact_rows=True, ctc_rows=ctc_rows, **kw)
    return gen.generate([model], {"net_input": {"source": wav, "padding_mask": pad}}, prefix_tokens=prefix_tokens)


def _golden_two(cuda):
    _, fx = load_golden("tiny_s2t_beam.pt")
    ni = to_dev(fx["samples"]["two"], cuda)["net_input"]
    wav, pad = ni["source"], ni["padding_mask"]
    lengths = (pad.size(1) - pad.sum(1)).tolist()
    return wav, pad, [wav[b, :n].contiguous() for b, n in enumerate(lengths)], lengths


# name -> (lengths in samples, seed of the waveforms); "two" is the two-sentence sample of tests/golden/tiny_s2t_beam.pt.
# Seeds picked on MI355X so that the single-sentence runs of the default path keep the margins (see the test's docstring).
BATCHES = {"two": None, "a": ([16000, 9000, 12345], 1), "b": ([8000, 16079, 11000, 6500], 4), "c": ([7000, 14000], 5)}
MAX_LEN_B = 12


def _load_batch(name, cuda):
    spec = BATCHES[name] if isinstance(name, str) else name
    if spec is None:
        return _golden_two(cuda)
    lengths, seed = spec
    wav, pad, clips = R.padded_batch(lengths, seed=seed, dtype=torch.float32)
    return wav.to(cuda), pad.to(cuda), [c.to(cuda) for c in clips], lengths


def _same_hypotheses(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} hypotheses, alone {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["tokens"].tolist() == w["tokens"].tolist(), f"{what} hypothesis {i}"
        assert abs(float(g["score"]) - float(w["score"])) <= SCORE_TOL * max(1.0, abs(float(w["score"]))), \
            (what, i, float(g["score"]), float(w["score"]))


def test_batched_ctc_rows_gives_single_sentence_hypotheses(cuda, tiny):
    """Every sentence of a batch decoded with exact_rows=True, ctc_rows=True against the default path on that sentence alone: all
    hypotheses, token for token and in order, scores within 2e-4 * max(1, |score|).  A case is compared when every decision of its
    single-sentence runs keeps MARGIN = 1e-4 (the margins are printed); at least three quarters of the cases, and at least eight,
    must be.  A case whose single-sentence run of the default path raises its KeyError has no reference and counts as left out.

    Measured on MI355X: 19 of 24 cases compared (two 5/6, a 4/6 with both beam-1 cases raising KeyError alone, b 6/6, c 4/6); the
    smallest margin of a compared case 1.19e-4, of the cases left out 3.8e-6 ... 9.3e-5; every compared case equal."""
    model, args, d = tiny
    layers = eval(args.conv_feature_layers)
    cases, kept = [], []
    for name in BATCHES:
        wav, pad, clips, lengths = _load_batch(name, cuda)
        assert MAX_LEN_B < min(R.frames(n, layers) for n in lengths)
        for beam in (1, 3, 4):
            for w in (0.3, 0.5):
                kw = dict(max_len_a=0, max_len_b=MAX_LEN_B, ctc_weight=w)
                singles, margin = [], dict(decision=float("inf"), ctc_list=float("inf"), hyps=float("inf"), all_adjacent=float("inf"))
                cases.append((name, beam, w))
                try:
                    for c in clips:
                        hyps, m = _single_run(model, d, c, beam, kw)
                        singles.append(hyps)
                        margin = {k: min(margin[k], m[k]) for k in margin}
                except KeyError:
                    # the default path itself gives up on a sentence (a token outside its CTC candidate list won): nothing to compare with
                    print(f"batch {name} beam {beam} ctc {w}: a single-sentence run raises KeyError -> left out")
                    continue
                ok = min(margin["decision"], margin["ctc_list"], margin["hyps"]) > MARGIN
                print(f"batch {name} beam {beam} ctc {w}: margins decision {margin['decision']:.3e} ctc list {margin['ctc_list']:.3e} "
                      f"hypotheses {margin['hyps']:.3e} (any adjacent {margin['all_adjacent']:.3e}) -> {'compared' if ok else 'left out'}")
                if ok:
                    kept.append((name, beam, w, wav, pad, singles, kw))
    assert len(kept) >= 8 and 4 * len(kept) >= 3 * len(cases), f"margins leave {len(kept)} of {len(cases)} cases"
    for name, beam, w, wav, pad, singles, kw in kept:
        got = _batched_run(model, d, wav, pad, beam, kw)
        for b, want in enumerate(singles):
            _same_hypotheses(got[b], want, f"batch {name} beam {beam} ctc {w} sentence {b}")


FEATURE_CASE = ("a", 3, 0.5)          # (batch, beam, ctc weight), found by seed on MI355X


def test_without_ctc_rows_a_batch_scores_against_sentence_zero(cuda, tiny):
    """Why the feature exists: in a batch the default path scores sentence 1 against sentence 0's posterior and returns another best
    hypothesis than for sentence 1 alone; with ctc_rows it returns that one."""
    model, _, d = tiny
    name, beam, w = FEATURE_CASE
    wav, pad, clips, _ = _load_batch(name, cuda)
    kw = dict(max_len_a=0, max_len_b=MAX_LEN_B, ctc_weight=w)
    alone, m = _single_run(model, d, clips[1], beam, kw)
    assert min(m["decision"], m["ctc_list"], m["hyps"]) > MARGIN, m
    off = _batched_run(model, d, wav, pad, beam, kw, ctc_rows=False)
    on = _batched_run(model, d, wav, pad, beam, kw, ctc_rows=True)
    assert off[1][0]["tokens"].tolist() != alone[0]["tokens"].tolist()
    _same_hypotheses(on[1], alone, "sentence 1 with ctc_rows")


class _CountingLib:
    def __init__(self, inner, log):
        self._inner, self._log = inner, log

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        if not name.startswith("st5_"):
            return fn

        def counted(*a):
            self._log.append(name)
            return fn(*a)
        return counted


def _count_lib_calls(fn):
    from speecht5_amd import hip
    log, inner = [], hip.lib
    proxy = _CountingLib(inner(), log)
    hip.lib = lambda: proxy
    try:
        out = fn()
    finally:
        hip.lib = inner
    return out, log


def test_default_path_makes_the_library_calls_it_made_before(cuda, tiny):
    """ctc_rows=False (the default): one st5_ctc_initial_state, one st5_ctc_prefix_score per decoder step and no rows entry; every
    other library call of the decode is what ctc_rows=True makes too, name for name and in order (the option touches the scorer
    only).  ctc_rows=True with ctc_weight == 0 does nothing."""
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _, d = tiny
    wav, pad, clips, _ = _golden_two(cuda)
    sample = {"net_input": {"source": wav[:1], "padding_mask": pad[:1]}}
    kw = dict(max_len_a=0, max_len_b=MAX_LEN_B, ctc_weight=0.5)
    steps = []
    inner = model.forward_decoder
    model.forward_decoder = lambda *a, **k: (steps.append(1), inner(*a, **k))[1]
    try:
        SequenceGenerator([model], d, beam_size=3, **kw).generate([model], sample)      # (first use fills the weight caches)
        steps.clear()
        assert SequenceGenerator([model], d, beam_size=3, **kw).ctc_rows is False
        h_off, off = _count_lib_calls(lambda: SequenceGenerator([model], d, beam_size=3, **kw).generate([model], sample))
        n_steps = len(steps)
        h_on, on = _count_lib_calls(lambda: SequenceGenerator([model], d, beam_size=3, ctc_rows=True, **kw).generate([model], sample))
    finally:
        del model.forward_decoder
    ctc_off = [n for n in off if n.startswith("st5_ctc_")]
    assert ctc_off == ["st5_ctc_initial_state"] + ["st5_ctc_prefix_score"] * n_steps and n_steps > 1
    ctc_on = [n for n in on if n.startswith("st5_ctc_")]
    assert ctc_on[0] == "st5_ctc_initial_state_rows" and sorted(set(ctc_on[1:])) == ["st5_ctc_prefix_score_rows", "st5_ctc_select_rows"]
    assert [n for n in off if not n.startswith("st5_ctc_")] == [n for n in on if not n.startswith("st5_ctc_")]
    _same_hypotheses(h_on[0], h_off[0], "one sentence, ctc_rows on against off")
    kw0 = dict(max_len_a=0, max_len_b=MAX_LEN_B, ctc_weight=0.0)
    h0, plain = _count_lib_calls(lambda: SequenceGenerator([model], d, beam_size=3, **kw0).generate([model], sample))
    h1, rows0 = _count_lib_calls(lambda: SequenceGenerator([model], d, beam_size=3, ctc_rows=True, **kw0).generate([model], sample))
    assert plain == rows0 and not [n for n in plain if n.startswith("st5_ctc_")]
    assert [h["tokens"].tolist() for h in h0[0]] == [h["tokens"].tolist() for h in h1[0]]


def test_ctc_rows_travels_through_build_generator(cuda, tiny):
    from argparse import Namespace
    from speecht5_amd.task import SpeechT5Task
    model, args, _ = tiny
    task = SpeechT5Task(args, Task().dicts)
    gen_args = Namespace(beam=1, max_len_a=0, max_len_b=6)
    assert task.build_generator([model], gen_args, extra_gen_cls_kwargs={"ctc_rows": True}).ctc_rows is True
    assert task.build_generator([model], gen_args).ctc_rows is False


# ((lengths, seed), beam, ctc weight): the middle sentence ends at 7 tokens, the others at 13; found on MI355X
SHRINK_CASE = (([16000, 9000, 12345], 3), 1, 0.5)


def test_a_sentence_that_leaves_the_batch_early(cuda, tiny):
    """One sentence finishes several steps before the others and leaves the batch (the rows, and ctc_sent with them, are renumbered):
    the sentences that stay get what they get alone."""
    model, _, d = tiny
    name, beam, w = SHRINK_CASE
    wav, pad, clips, _ = _load_batch(name, cuda)
    kw = dict(max_len_a=0, max_len_b=MAX_LEN_B, ctc_weight=w)
    singles, margins = [], []
    for c in clips:
        hyps, m = _single_run(model, d, c, beam, kw)
        singles.append(hyps)
        margins.append(min(m["decision"], m["ctc_list"], m["hyps"]))
    ends = [max(len(h["tokens"]) for h in hyps) for hyps in singles]
    print("last hypothesis of each sentence ends at", ends, "margins", " ".join(f"{m:.3e}" for m in margins))
    assert min(margins) > MARGIN
    assert min(ends) + 3 <= max(ends) and ends.index(min(ends)) != len(ends) - 1, ends      # (rows behind it are renumbered)
    got = _batched_run(model, d, wav, pad, beam, kw)
    for b, want in enumerate(singles):
        _same_hypotheses(got[b], want, f"sentence {b}")
