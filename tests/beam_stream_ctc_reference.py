"""numpy restatement of the per-slot CTC step of a beam-search stream with joint CTC / attention scoring (include/speecht5_hip.h:
st5_beam_ctc_candidates_sents, st5_ctc_prefix_score_rows_sents, st5_beam_step_sents_logprobs, st5_ctc_select_sents,
st5_ctc_sents_admit; speecht5_amd/beam_stream.py, joint_ctc), built from tests/beam_ctc_reference.py (candidates, mix, select),
tests/ctc_rows_reference.py (the prefix scores) and tests/beam_stream_reference.py (BeamStreamRef: the per-slot beam step).  TEST
INFRASTRUCTURE: tests/test_beam_stream_ctc_cpu.py holds every slot to the scalar restatement at the slot's own step.

Slot s owns rows s*beam .. s*beam+beam-1 of every array, its slice of the posterior x [n_slots, S, V] and frames[s], unknown[s].  A
step takes the UNRULED log-probabilities of the rows (what the candidates kernel computes from the logits).

`faults`: names of planted faults, each a way the per-slot step can be wrong."""
import numpy as np

from tests import beam_ctc_reference as R
from tests.beam_step_reference import BeamStepRef
from tests.beam_stream_reference import BeamStreamRef
from tests.ctc_reference import LOGZERO
from tests.ctc_rows_reference import rows_initial, rows_score

FAULTS = ("done_slot_writes", "select_unmoved", "admit_keeps_unknown", "admit_keeps_prev", "admit_keeps_frames")
POISON = np.float32(-7.25e30)


def ctc_scores(x, T, blank, eos, step, last, cs, state):
    """log_psi [n, nc] and r_new [n, S, nc, 2] of the rows of ONE sentence (posterior x [S, V], T frames) at out_len = step."""
    n = cs.shape[0]
    if T <= 0:                                             # (a slot without frames: nothing to walk, every extension is impossible)
        return np.full(cs.shape, LOGZERO, np.float32), np.zeros((n, 0) + cs.shape[1:] + (2,), np.float32)
    log_psi, r = rows_score(x[None], [T], np.zeros(n, np.int64), last, step, cs, state, blank, eos, np.float32)
    return log_psi.astype(np.float32), np.ascontiguousarray(np.transpose(r, (0, 2, 1, 3))).astype(np.float32)


class ScalarCtcRef:
    """The scalar step (beam_graph.py's CTC step) of ONE sentence: BeamStepRef with the CTC part of beam_ctc_reference around it."""

    def __init__(self, x, T, beam, V, nc, max_len, w, blank, never, **rules):
        self.bs = BeamStepRef(1, beam, V, max_len, rules["eos"], never=never, **rules)
        self.x, self.T, self.nc, self.w, self.blank, self.eos, self.never = np.asarray(x, np.float32), int(T), nc, w, blank, rules["eos"], never
        S = self.x.shape[0]
        self.state = np.repeat(rows_initial(self.x[None], [self.T], blank, np.float32), beam, 0)
        self.r_new = np.full((beam, S, nc, 2), POISON, np.float32)
        self.log_psi = np.full((beam, nc), POISON, np.float32)
        self.cs = np.full((beam, nc), -1, np.int32)
        self.lp = np.full((beam, V), POISON, np.float32)
        self.prev = np.zeros(beam, np.float32)
        self.unknown = 0

    def step(self, logp):
        bs = self.bs
        step = bs.counter
        if step > bs.max_len:
            return
        self.cs = R.candidates(logp, self.never, self.nc)
        self.log_psi, self.r_new = ctc_scores(self.x, self.T, self.blank, self.eos, step, bs.tok[:, step], self.cs, self.state)
        self.lp = R.mix(logp, self.cs, self.log_psi, self.prev, self.w)
        bs.step(self.lp)
        t = bs.counter
        if 1 <= t <= bs.max_len:
            self.state, self.prev, unk = R.select(bs.parent, bs.tok[:, t], self.cs, self.log_psi, self.r_new, [self.T], bs.beam, bs.ignore,
                                                  bs.sent_done)
            self.unknown |= unk
        bs.reorder()

    def arrays(self):
        return dict(cs=self.cs, lp=self.lp, log_psi=self.log_psi, r_new=self.r_new[:, :self.T], state=self.state, prev=self.prev,
                    unknown=np.int32(self.unknown))


class BeamStreamCtcRef:
    def __init__(self, n_slots, beam, V, cap, S, nc, w, blank, never, *, faults=(), **rules):
        assert all(f in FAULTS for f in faults)
        self.ref = BeamStreamRef(n_slots, beam, V, cap, S=S, never=never, **rules)
        self.faults = set(faults)
        self.n_slots, self.beam, self.V, self.S, self.nc, self.w, self.blank, self.eos, self.never = (n_slots, beam, V, S, nc, w, blank,
                                                                                                      rules["eos"], never)
        rows = n_slots * beam
        self.x = np.zeros((n_slots, S, V), np.float32)
        self.frames = np.zeros(n_slots, np.int32)
        self.state = np.full((rows, S, 2), LOGZERO, np.float32)
        self.r_new = np.full((rows, S, nc, 2), POISON, np.float32)
        self.log_psi = np.full((rows, nc), POISON, np.float32)
        self.prev = np.zeros(rows, np.float32)
        self.cs = np.full((rows, nc), -1, np.int32)
        self.lp = np.full((rows, V), POISON, np.float32)
        self.unknown = np.zeros(n_slots, np.int32)

    def admit(self, slot, max_len, frames, bos, post):
        if not 0 <= slot < self.n_slots:
            return
        self.ref.admit(slot, max_len, frames, bos)
        T = min(max(int(frames), 0), self.S)
        b0, b1 = slot * self.beam, (slot + 1) * self.beam
        self.x[slot, :T] = np.asarray(post, np.float32)[:T]
        if "admit_keeps_frames" not in self.faults:
            self.frames[slot] = T
        T = int(self.frames[slot])
        self.state[b0:b1] = np.repeat(rows_initial(self.x[slot:slot + 1], [T], self.blank, np.float32), self.beam, 0)
        if "admit_keeps_prev" not in self.faults:
            self.prev[b0:b1] = 0
        if "admit_keeps_unknown" not in self.faults:
            self.unknown[slot] = 0

    def step(self, logp):
        """logp [rows, V]: unruled log-probabilities; the rows of done slots are never read."""
        ref, beam = self.ref, self.beam
        logp = np.asarray(logp, np.float32)
        for s in range(self.n_slots):
            in_range = 0 <= ref.pos[s] <= ref.maxlen[s]
            if not (ref.live(s) or ("done_slot_writes" in self.faults and in_range)):
                continue                                   # (before the first load: lp, cs, log_psi, r_new keep their bytes)
            b0, b1 = s * beam, (s + 1) * beam
            step, T = int(ref.pos[s]), int(self.frames[s])
            self.cs[b0:b1] = R.candidates(logp[b0:b1], self.never, self.nc)
            self.log_psi[b0:b1], r_new = ctc_scores(self.x[s], T, self.blank, self.eos, step, ref.tok[b0:b1, step], self.cs[b0:b1],
                                                    self.state[b0:b1])
            self.r_new[b0:b1, :T] = r_new[:, :T]           # (frames behind the sentence's are not written)
            self.lp[b0:b1] = R.mix(logp[b0:b1], self.cs[b0:b1], self.log_psi[b0:b1], self.prev[b0:b1], self.w)
        ref.step(self.lp)
        for s in range(self.n_slots):
            t = int(ref.pos[s])
            if not (ref.moved[s] or "select_unmoved" in self.faults) or t < 1 or t > ref.maxlen[s]:
                continue
            b0, b1 = s * beam, (s + 1) * beam
            T = int(self.frames[s])
            r_new = np.where(np.arange(self.S)[None, :, None, None] < T, self.r_new[b0:b1], np.float32(LOGZERO))
            self.state[b0:b1], self.prev[b0:b1], unk = R.select(ref.parent[b0:b1] - b0, ref.tok[b0:b1, t], self.cs[b0:b1],
                                                                self.log_psi[b0:b1], r_new, [T], beam, ref.ignore[b0:b1], ref.done[s:s + 1])
            if unk:
                self.unknown[s] = 1
        ref.reorder()

    def arrays(self, s):
        """The compared arrays of slot s (r_new over its live frames)."""
        b0, b1 = s * self.beam, (s + 1) * self.beam
        return dict(cs=self.cs[b0:b1], lp=self.lp[b0:b1], log_psi=self.log_psi[b0:b1], r_new=self.r_new[b0:b1, :self.frames[s]],
                    state=self.state[b0:b1], prev=self.prev[b0:b1], unknown=self.unknown[s])

    def snapshot(self):
        return b"".join(np.ascontiguousarray(a).tobytes() for a in (self.frames, self.state, self.r_new, self.log_psi, self.prev, self.cs,
                                                                    self.lp, self.unknown))
