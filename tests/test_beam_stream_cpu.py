"""The beam-search stream (speecht5_amd/beam_stream.py, st5_beam_*_sents) without a GPU:
1. the numpy restatement of the per-sentence step (tests/beam_stream_reference.py) driven as a whole stream over the fake model of
   tests/fake_seq_model.py: every request's hypotheses equal the existing CPU generator's for that sentence ALONE (tokens identical,
   scores and positional scores bit-equal), whatever slot, admission tick and neighbours it had;
2. completion order, polls and tick count equal tts_stream.stream_schedule on the singles' step counts;
3. planted faults are caught: a done slot that advances, a reorder applied to an unmoved slot, an admit that leaves an old ignore
   flag, an admit that leaves an old record count;
4. csrc/beam_stream_index.h compiled with the host compiler into a stand-alone program and swept."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests.beam_stream_reference import FAULTS, BeamStreamRef, simulate_stream
from tests.fake_seq_model import FakeSeqModel
from tests.util import Task

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_SLOTS, POLL, MAX_SRC = 3, 4, 1600
KW = dict(beam_size=3, max_len_b=14, len_penalty=1.2)
# (samples, max_len): multiples of the fake encoder's hop; None: the generator's own formula
REQUESTS = [(1600, 14), (400, 3), (960, 9), (480, 5), (1280, None), (800, 6), (640, 11), (1120, 2), (560, 7)]


def _requests(seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(f"utt{i}", torch.randn(n, generator=g), ml) for i, (n, ml) in enumerate(REQUESTS)]


def _gen(**kw):
    from speecht5_amd.sequence_generator import SequenceGenerator
    d = Task().dicts["text"]
    model = FakeSeqModel(len(d), seed=3).eval()
    return SequenceGenerator([model], d, **(KW | kw)), model


def _single(model, src, limit):
    """The existing generator on one sentence alone, with the request's step limit."""
    from speecht5_amd.sequence_generator import SequenceGenerator
    gen = SequenceGenerator([model], Task().dicts["text"], **(KW | dict(max_len_b=limit, max_len_a=0)))
    sample = {"net_input": {"source": src.unsqueeze(0), "padding_mask": torch.zeros(1, src.numel(), dtype=torch.bool)}}
    return gen.generate([model], sample)[0]


def _steps_of(hyps, beam, limit):
    """Steps a sentence runs: one more than the step of its `beam`-th hypothesis, or of the limit."""
    return (max(len(h["tokens"]) for h in hyps) - 1 if len(hyps) == beam else limit) + 1


@pytest.fixture(scope="module")
def stream():
    gen, model = _gen()
    reqs = _requests()
    with torch.no_grad():
        out, ticks, polls, steps, ref = simulate_stream(gen, reqs, N_SLOTS, MAX_SRC, POLL)
        singles = {key: _single(model, src, ml if ml is not None else KW["max_len_b"]) for key, src, ml in reqs}
    return gen, reqs, out, ticks, polls, steps, ref, singles


def _same(a, b):
    return (a["tokens"].tolist() == b["tokens"].tolist()
            and np.float32(a["score"]).tobytes() == b["score"].numpy().astype(np.float32).tobytes()
            and a["positional_scores"].tobytes() == b["positional_scores"].numpy().astype(np.float32).tobytes())


def test_every_request_equals_the_generator_on_the_sentence_alone(stream):
    _, reqs, out, _, _, _, ref, singles = stream
    assert ref.min_gap > 0, "an exact tie among the finite candidates (torch.topk has no tie rule: pick another seed)"
    assert sorted(k for k, _ in out) == sorted(k for k, _, _ in reqs)
    for key, hyps in out:
        want = singles[key]
        assert len(hyps) == len(want) > 0, key
        for hi, (a, b) in enumerate(zip(hyps, want)):
            assert _same(a, b), (key, hi)


def test_completion_order_and_ticks_follow_stream_schedule(stream):
    from speecht5_amd.tts_stream import stream_schedule
    gen, reqs, out, ticks, polls, steps, _, singles = stream
    lengths = [_steps_of(singles[key], gen.beam_size, ml if ml is not None else KW["max_len_b"]) for key, _, ml in reqs]
    assert [steps[key] for key, _, _ in reqs] == lengths
    want_ticks, order, plan = stream_schedule(lengths, N_SLOTS, POLL, with_plan=True)
    assert ticks == want_ticks and polls == want_ticks // POLL
    assert [k for k, _ in out] == [reqs[i][0] for i in order]
    # the inputs are not trivial: several finishing steps, a sentence ended by eos before its limit, a reused slot, two at one poll
    assert len(set(lengths)) >= 3
    assert any(n < (ml if ml is not None else KW["max_len_b"]) + 1 for n, (_, _, ml) in zip(lengths, reqs))
    assert len(plan) > N_SLOTS
    ends = [(t + lengths[i] + POLL - 1) // POLL for i, _, t in plan]
    assert len(set(ends)) < len(ends)


# ---- planted faults: a scripted two-slot sequence whose state must differ, or a stream whose results must ----
RULES = dict(pad=1, unk=3, eos=2, min_len=1, len_penalty=1.0)


def _scripted(faults=()):
    """Slot 0 (beam 2, limit 5) collects its two hypotheses at step 1 with its rows' parents swapped and then waits, done, for one
    more tick while slot 1 runs on; then it is handed to a new sentence.  Returns the bytes of everything."""
    V, beam = 11, 2
    ref = BeamStreamRef(2, beam, V, 5, S=4, faults=faults, **RULES)
    ref.admit(0, 5, 3, 2)
    ref.admit(1, 4, 4, 2)
    lp0 = np.full((4, V), -9.0, np.float32)
    lp0[:, 5], lp0[:, 6] = -1.0, -1.2
    ref.step(lp0)
    ref.reorder()
    lp1 = np.full((4, V), -9.0, np.float32)
    lp1[0, 2], lp1[0, 5] = -0.1, -3.0                 # slot 0: eos of both rows first, then (row 1, 6), (row 0, 5): parents [1, 0]
    lp1[1, 2], lp1[1, 6] = -0.1, -0.5
    lp1[2:, 7], lp1[2:, 8] = -1.0, -1.5
    ref.step(lp1)
    ref.reorder()
    assert ref.done.tolist() == [1, 0] and ref.n_hyp.tolist() == [2, 0] and ref.parent[:2].tolist() == [1, 0]
    ref.ignore[:2] = True                             # (flags an occupant may leave behind)
    f = ref.full
    snap = lambda: b"".join(np.ascontiguousarray(a).tobytes() for a in (                             # noqa: E731
        f.tok, f.score, f.anc, f.ignore, f.rec_tok, f.rec_pos, f.rec_score, f.rec_len, f.n_hyp, ref.pos, ref.pos_rows, ref.maxlen, ref.done,
        ref.moved, ref.kpm))
    ref.step(lp1)
    ref.reorder()
    waiting = snap()                                  # (the hand-over resets the ancestry rows: the done slot is looked at before it)
    ref.admit(0, 3, 2, 2)
    return waiting + snap()


def test_scripted_sequence_leaves_a_done_slot_alone():
    V, beam = 11, 2
    ref = BeamStreamRef(2, beam, V, 5, S=4, **RULES)
    ref.admit(0, 0, 3, 2)                              # limit 0: finished by its first step
    ref.admit(1, 4, 4, 2)
    lp = np.log(np.random.default_rng(0).dirichlet(np.ones(V), 4)).astype(np.float32)
    ref.step(lp)
    ref.reorder()
    assert ref.done.tolist() == [1, 0] and ref.moved.tolist() == [1, 1] and ref.pos.tolist() == [1, 1]
    f = ref.full
    before = [a[:beam].copy() for a in (f.tok, f.score, f.anc, f.ignore, f.rec_tok, f.rec_pos, f.rec_score, f.rec_len)] + [ref.pos.copy()]
    ref.step(lp)
    ref.reorder()
    after = [a[:beam] for a in (f.tok, f.score, f.anc, f.ignore, f.rec_tok, f.rec_pos, f.rec_score, f.rec_len)] + [ref.pos]
    assert ref.moved.tolist() == [0, 1] and ref.pos.tolist() == [1, 2]
    assert all(np.array_equal(a, b) for a, b in zip(after[:-1], before[:-1]))


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_caught(stream, fault):
    caught = _scripted(faults=(fault,)) != _scripted()
    if not caught:
        gen, reqs, out, ticks, _, steps, _, _ = stream
        with torch.no_grad():
            out2, ticks2, _, steps2, _ = simulate_stream(gen, reqs, N_SLOTS, MAX_SRC, POLL, faults=(fault,))
        caught = ticks2 != ticks or steps2 != steps or [k for k, _ in out2] != [k for k, _ in out] or any(
            len(a) != len(b) or not all(x["tokens"].tolist() == y["tokens"].tolist() and x["score"] == y["score"] for x, y in zip(a, b))
            for (_, a), (_, b) in zip(out2, out))
    assert caught, f"planted fault {fault!r} went unnoticed"


def test_stream_catches_an_admit_that_keeps_the_record_count(stream):
    """Not only the scripted state: the stream's results themselves are wrong when a slot's old record count survives its hand-over."""
    gen, reqs, out, _, _, _, _, _ = stream
    with torch.no_grad():
        out2, _, _, _, _ = simulate_stream(gen, reqs, N_SLOTS, MAX_SRC, POLL, faults=("admit_keeps_n_hyp",))
    a, b = dict(out), dict(out2)
    assert any(len(a[k]) != len(b.get(k, ())) or any(x["tokens"].tolist() != y["tokens"].tolist() for x, y in zip(a[k], b[k])) for k in a)


# ---- the index header on the host ----
SWEEP = r"""
#include <cstdio>
#include "beam_stream_index.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d) cap=%d raw=%d pos=%d beam=%d slot=%d\n", #c, __LINE__, cap, raw, pos, beam, slot); return 1; } } while (0)
int main() {
  int cap = 0, raw = 0, pos = 0, beam = 0, slot = 0;
  long long cases = 0;
  const int beams[4] = {1, 2, 5, 32};
  for (cap = 0; cap <= 6; ++cap) for (raw = -2; raw <= cap + 3; ++raw) for (pos = -2; pos <= cap + 3; ++pos) {
    const int Tmax = cap + 2, rec_ld = cap + 1, pos_rows = Tmax + 4;
    const int want = raw < 0 ? 0 : (raw > cap ? cap : raw);
    const int m = bst_maxlen(raw, cap);
    CHECK(m == want && m >= 0 && m <= cap);
    const bool live = bst_step_live(pos, m);
    CHECK(live == (pos >= 0 && pos <= m));
    if (live) {
      CHECK(pos < rec_ld);                                      // the record's last column and the len_div entry of the step
      if (pos < m) CHECK(bst_next_col(pos) == pos + 1 && bst_next_col(pos) < Tmax - 1);   // tok / score of the continuing rows
      CHECK(bst_next_col(pos) <= Tmax - 1);                     // the position the slot is left at: a K|V slot and a token column
    }
    const long long n = bst_reorder_cols(pos, m, Tmax);
    CHECK(n == ((pos >= 1 && pos <= m) ? pos : 0) && n >= 0 && n <= Tmax);
    const int col = bst_embed_col(pos, Tmax);
    CHECK(col >= 0 && col <= Tmax - 1 && (pos < 0 || pos > Tmax - 1 || col == pos));
    for (int off = -3; off <= 3; ++off) { const int pr = bst_pos_row(col, off, pos_rows); CHECK(pr >= 0 && pr < pos_rows); }
    for (int n_hyp = 0; n_hyp <= 3; ++n_hyp) CHECK(bst_finished(n_hyp, 3, pos, m) == (n_hyp == 3 || pos == m));
    ++cases;
  }
  // the admission: every write of a slot lies inside the slot, a slot outside the stream admits nothing
  const int n_slots = 3;
  cap = 4; raw = pos = 0;
  for (int bi = 0; bi < 4; ++bi) for (slot = -1; slot <= n_slots; ++slot) for (int S = 1; S <= 7; S += 3) for (int frames = -1; frames <= S + 1; ++frames) {
    beam = beams[bi];
    const int Tmax = cap + 2;
    const long long anc_ld = Tmax + 3;
    CHECK(bst_slot_ok(slot, n_slots) == (slot >= 0 && slot < n_slots));
    if (!bst_slot_ok(slot, n_slots)) continue;
    const long long row0 = bst_row0(slot, beam);
    CHECK(row0 == (long long)slot * beam);
    for (int b = 0; b < beam; ++b) for (int j = 0; j < Tmax; ++j) {
      const long long a = bst_cell_off(row0 + b, anc_ld, j), t = bst_cell_off(row0 + b, Tmax, j);
      CHECK(a >= row0 * anc_ld && a < (row0 + beam) * anc_ld && a - (row0 + b) * anc_ld == j);
      CHECK(t >= row0 * Tmax && t < (row0 + beam) * Tmax);
    }
    const int fr = bst_frames(frames, S);
    CHECK(fr == (frames < 0 ? 0 : (frames > S ? S : frames)));
    int valid = 0;
    for (int j = 0; j < S; ++j) {
      const long long k = bst_kpm_off(slot, S, j);
      CHECK(k >= (long long)slot * S && k < (long long)(slot + 1) * S);
      CHECK(bst_kpm_byte(j, fr) == (j >= fr ? 1 : 0));
      valid += bst_kpm_byte(j, fr) ? 0 : 1;
    }
    CHECK(valid == fr);
    ++cases;
  }
  // values of the cells that do not fit on the way in; offsets past 2^31
  cap = 7; beam = 32; slot = 65534;
  raw = 2147483647; CHECK(bst_maxlen(raw, cap) == 7);
  raw = -2147483647 - 1; CHECK(bst_maxlen(raw, cap) == 0 && !bst_step_live(raw, 7));
  CHECK(bst_cell_off(bst_row0(slot, beam) + 31, 1LL << 20, 5) == ((65534LL * 32 + 31) << 20) + 5);
  CHECK(bst_embed_col(2147483647, 9) == 8 && bst_embed_col(-2147483647 - 1, 9) == 0);
  CHECK(bst_pos_row(2147483647, 2147483647, 12) == 11);
  std::printf("OK %lld cases\n", cases);
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_index_header_sweep_on_the_host(tmp_path):
    src = tmp_path / "sweep.cpp"
    src.write_text(SWEEP)
    exe = tmp_path / "sweep"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "speecht5_amd", "csrc"), str(src),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    n_state = sum((cap + 6) ** 2 for cap in range(7))
    n_admit = 4 * 3 * sum(S + 3 for S in (1, 4, 7))
    assert r.stdout.split()[1] == str(n_state + n_admit)
