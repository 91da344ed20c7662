"""Joint CTC / attention scoring in the beam-search stream (speecht5_amd/beam_stream.py joint_ctc, the st5_*_sents entries of
csrc/beam_ctc.hip) without a GPU:
1. the per-slot index arithmetic of csrc/beam_stream_index.h compiled with the host compiler into a stand-alone program and swept;
2. the numpy restatement of the per-slot CTC step (tests/beam_stream_ctc_reference.py): each slot equals the scalar restatement of
   one sentence at the slot's own step, whatever its neighbours do, through staggered admissions, a done slot and a dirty hand-over;
3. planted faults each change a compared array: a done slot that writes, a select on an unmoved slot, an admit that leaves an old
   `unknown`, `prev` or `frames`;
4. beam_stream.check_arguments accepts and refuses as generate_stream documents."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests.beam_stream_ctc_reference import FAULTS, BeamStreamCtcRef, ScalarCtcRef
from tests.util import Task, build_tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the index header on the host ----
SWEEP = r"""
#include <cstdio>
#include "beam_stream_index.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d) a=%d b=%d c=%d d=%d\n", #c, __LINE__, a, b, c, d); return 1; } } while (0)
int main() {
  int a = 0, b = 0, c = 0, d = 0;
  long long cases = 0;
  // the gates: a = done, b = pos, c = raw maxlen, d = moved; cap = 4
  const int cap = 4;
  for (a = 0; a <= 2; ++a) for (b = -2; b <= cap + 3; ++b) for (c = -2; c <= cap + 3; ++c) for (d = 0; d <= 2; ++d) {
    const int m = bst_maxlen(c, cap);
    const bool live = bst_ctc_live(a, b, m);
    CHECK(live == (a == 0 && b >= 0 && b <= m));
    if (live) CHECK(b <= cap);                                   // tok[r][pos]: a column below Tmax = cap + 2
    const bool sel = bst_select_live(d, b, m);
    CHECK(sel == (d != 0 && b >= 1 && b <= m));
    if (sel) CHECK(b < cap + 2);                                 // tok[r][t]
    // the select behind a live step acts exactly when that step wrote continuing rows (step < maxlen)
    if (live) CHECK(bst_select_live(1, bst_next_col(b), m) == (b < m));
    ++cases;
  }
  // rows, parents and offsets: a = n_slots, b = beam, c = slot, d = S; every cell of a slot lies inside the slot's rows
  const int beams[4] = {1, 2, 5, 32};
  const int V = 41, nc = 7;
  for (a = 1; a <= 3; ++a) for (int bi = 0; bi < 4; ++bi) for (c = 0; c < a; ++c) for (d = 1; d <= 37; d += 12) {
    b = beams[bi];
    const long long rows = (long long)a * b, row0 = bst_row0(c, b);
    for (long long r = row0; r < row0 + b; ++r) {
      CHECK(bst_slot_of(r, b) == c);
      for (long long p = -1; p <= rows; ++p) CHECK(bst_parent_ok(p, c, b) == (p >= row0 && p < row0 + b));
      const long long st = bst_state_off(r, d);
      CHECK(st == r * d && st >= row0 * d && st + d <= (row0 + b) * (long long)d);
      for (int j = 0; j < nc; ++j) {
        const long long rn = bst_rnew_off(r, d, nc, j), cell = bst_cand_off(r, nc, j);
        CHECK(rn + (long long)(d - 1) * nc < (row0 + b) * (long long)d * nc && rn >= row0 * (long long)d * nc);
        CHECK(cell >= row0 * nc && cell < (row0 + b) * nc);
      }
    }
    const long long x0 = bst_x_off(c, d, V);
    CHECK(x0 == (long long)c * d * V && x0 + (long long)d * V <= (long long)a * d * V);
    for (int fr = -1; fr <= d + 1; ++fr) { const int T = bst_frames(fr, d); CHECK(T >= 0 && T <= d); }
    ++cases;
  }
  a = b = c = d = 0;
  for (int t = -2; t <= V + 1; ++t) CHECK(bst_token_ok(t, V) == (t >= 0 && t < V));
  // offsets past 2^31: 192 rows x 8000 frames x 224 candidates
  CHECK(bst_rnew_off(191, 8000, 224, 223) == 191LL * 8000 * 224 + 223);
  CHECK(bst_x_off(5, 8000, 100000) == 5LL * 8000 * 100000);
  CHECK(!bst_ctc_live(0, 2147483647, 4) && !bst_select_live(1, -2147483647 - 1, 4) && !bst_parent_ok(2147483647, 0, 32));
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
    assert r.stdout.split()[1] == str(3 * 10 * 10 * 3 + sum(a * 4 * 4 for a in (1, 2, 3)))


# ---- the restatement: every slot is the scalar step at its own position ----
N_SLOTS, BEAM, V, CAP, S, NC, W = 3, 2, 13, 4, 9, 5, 0.3
BLANK, PAD, EOS, UNK = 0, 1, 2, 3
FRAMES = (9, 5, 1)
RULES = dict(pad=PAD, unk=UNK, eos=EOS, min_len=1, len_penalty=1.0)
ADMIT_TICK = {2: 0, 1: 2, 0: 4}                    # before tick 4 runs: pos = (0, 2, maxlen = 4)
TICKS = 7


def _never():
    never = np.zeros(V, bool)
    never[BLANK] = True
    return never


def _inputs():
    g = torch.Generator().manual_seed(7)
    x = torch.log_softmax(torch.randn(N_SLOTS, S, V, generator=g) * 2, -1).numpy()
    logits = torch.randn(TICKS, N_SLOTS * BEAM, V, generator=g) * 3
    logits[:, :, EOS] -= 8.0                                        # (most sentences run to their limit)
    logits[4, BEAM:2 * BEAM, EOS] += 60.0                           # (slot 1 collects its hypotheses at its step 2, below its limit)
    return x, torch.log_softmax(logits, -1).numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _run(faults=(), check=False):
    """Three slots admitted at ticks 0, 2, 4 (each handed over dirty), stepped for TICKS ticks; slot 2 is done behind tick 4 (at its
    limit) and is handed to a second sentence at tick 6; slot 1 is done behind tick 4 too, by eos at its step 2.  Returns the
    snapshots behind every tick."""
    x, logp = _inputs()
    st = BeamStreamCtcRef(N_SLOTS, BEAM, V, CAP, S, NC, W, BLANK, _never(), faults=faults, **RULES)
    single, snaps = {}, []

    def admit(s):
        b0, b1 = s * BEAM, (s + 1) * BEAM
        st.state[b0:b1], st.prev[b0:b1], st.unknown[s], st.frames[s] = np.nan, 5.0, 1, 4       # what an occupant may leave behind
        st.admit(s, CAP, FRAMES[s], EOS, x[s, :FRAMES[s]])
        single[s] = (ScalarCtcRef(x[s], FRAMES[s], BEAM, V, NC, CAP, W, BLANK, _never(), **RULES), 0)

    for tick in range(TICKS):
        for s, t0 in ADMIT_TICK.items():
            if t0 == tick:
                admit(s)
        if tick == 6:
            assert st.ref.done[2] == 1
            admit(2)
        if tick == 4:
            assert st.ref.pos.tolist() == [0, 2, CAP] and st.ref.done.tolist() == [0, 0, 0]
        if tick == 5:
            assert st.ref.done.tolist() == [0, 1, 1] and st.ref.pos.tolist() == [1, 3, CAP + 1]
            st.state[BEAM:2 * BEAM] = 123.0                         # (a finished slot inside its limit: nothing may touch it again)
        done_before = {s: {k: v.copy() for k, v in st.arrays(s).items()} for s in range(N_SLOTS) if st.ref.done[s]}
        st.step(logp[tick])
        for s in single:
            single[s][0].step(logp[tick][s * BEAM:(s + 1) * BEAM])
        snaps.append(st.snapshot() + st.ref.tok.tobytes() + st.ref.done.tobytes())
        if check:
            for s in range(N_SLOTS):
                got = st.arrays(s)
                if s in done_before:                                # a done (or idle) slot changes no byte of any CTC buffer
                    assert all(np.array_equal(_bits(got[k]), _bits(done_before[s][k])) for k in got), (tick, s)
                elif s in single:
                    want = single[s][0].arrays()
                    for k in want:
                        assert np.array_equal(_bits(got[k]), _bits(want[k])), (tick, s, k)
                    bs = single[s][0].bs
                    b0 = s * BEAM
                    n = bs.counter + 1                              # (columns behind the position may hold an earlier occupant's)
                    assert np.array_equal(st.ref.tok[b0:b0 + BEAM, :n], bs.tok[:, :n]) and int(st.ref.pos[s]) == bs.counter
                    assert np.array_equal(_bits(st.ref.score[b0:b0 + BEAM, :n]), _bits(bs.score[:, :n]))
    return snaps


def test_each_slot_equals_the_scalar_restatement_at_its_own_step():
    snaps = _run(check=True)
    assert len(set(snaps)) == TICKS and _run() == snaps, "the scenario moves at every tick and is deterministic"


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_changes_a_compared_array(fault):
    assert _run(faults=(fault,)) != _run(), f"planted fault {fault!r} went unnoticed"


# ---- the argument checks ----
@pytest.fixture(scope="module")
def tiny():
    model, _ = build_tiny(torch.device("cpu"), torch.float32)
    model.eval()
    return model, Task().dicts["text"]


def test_check_arguments_accepts_and_refuses(tiny):
    from speecht5_amd.beam_stream import check_arguments
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, d = tiny
    ok = dict(sentences=3, max_src_len=7000, decode="graph")
    gen = SequenceGenerator([model], d, beam_size=2, max_len_b=20, ctc_weight=0.4, ctc_rows=True)
    S, cap = check_arguments(gen, joint_ctc=True, **ok)
    assert S == int(model.speech_encoder_prenet._frames(7000)) and cap == 20
    assert check_arguments(SequenceGenerator([model], d, beam_size=2, max_len_b=20), **ok) == (S, cap)
    with pytest.raises(ValueError, match="ctc_weight.*joint_ctc"):                   # without the keyword the refusal stands
        check_arguments(gen, **ok)
    with pytest.raises(ValueError, match="ctc_weight.*joint_ctc"):
        check_arguments(SequenceGenerator([model], d, beam_size=2, ctc_weight=0.4), **ok)
    with pytest.raises(ValueError, match="joint_ctc"):
        check_arguments(SequenceGenerator([model], d, beam_size=2, max_len_b=20), joint_ctc=True, **ok)
    with pytest.raises(ValueError, match="ctc_rows"):
        check_arguments(SequenceGenerator([model], d, beam_size=2, ctc_weight=0.4), joint_ctc=True, **ok)
    with pytest.raises(ValueError, match="lm_model"):
        check_arguments(SequenceGenerator([model], d, beam_size=2, lm_model=torch.nn.Identity(), ctc_weight=0.4, ctc_rows=True),
                        joint_ctc=True, **ok)
    proj, model.encoder.proj = model.encoder.proj, None
    try:
        with pytest.raises(ValueError, match="CTC projection"):
            check_arguments(gen, joint_ctc=True, **ok)
    finally:
        model.encoder.proj = proj
    for kw, word in [(dict(ok, sentences=0), "sentences"), (dict(ok, sentences=17), "sentences"), (dict(ok, decode="slots"), "decode")]:
        with pytest.raises(ValueError, match=word):
            check_arguments(gen, joint_ctc=True, **kw)
