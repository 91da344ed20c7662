"""numpy restatement of the st5_beam_step contract (include/speecht5_hip.h, csrc/beam_step.hip), steps 2-6: the rules, the top
2 * beam candidates under the TIE RULE (higher score first; among equal scores, -inf included, the lower flat index
beam_row * V + token), the generator's EOS / continuation / cands_to_ignore logic, finalisation into per-sentence records, the
continuing rows in slot layout, and the in-place ancestry reorder.  Sentences never leave the batch.  TEST INFRASTRUCTURE: fed with
fp32 log-probabilities (ruled or unruled); tests/test_beam_step_cpu.py holds it to the existing generator, tests/test_beam_step_gpu.py
holds the kernel to it.

`faults`: names of planted faults, each a way the step can be wrong (test_beam_step_cpu.py shows that every one is caught)."""
import numpy as np

FAULTS = ("step0_all_beams", "eos_below_min_len", "ignored_slot_finalised", "normalise_by_step", "finished_sentence_leaks",
          "tie_higher_index_first")
NEG = np.float32(-np.inf)


class BeamStepRef:
    def __init__(self, n_sent, beam, V, max_len, bos, *, pad, unk, eos, unk_penalty=0.0, min_len=1, normalize_scores=True,
                 len_penalty=1.0, never=None, faults=()):
        assert beam <= 32 and V - 1 >= 2 * beam and all(f in FAULTS for f in faults)
        self.n_sent, self.beam, self.V, self.max_len = n_sent, beam, V, max_len
        self.pad, self.unk, self.eos, self.unk_penalty, self.min_len = pad, unk, eos, np.float32(unk_penalty), min_len
        self.normalize_scores, self.len_penalty = normalize_scores, len_penalty
        self.never = np.zeros(V, bool) if never is None else np.asarray(never).astype(bool)
        self.faults = set(faults)
        rows, Tmax = n_sent * beam, max_len + 2
        self.rows, self.Tmax = rows, Tmax
        self.counter = 0
        self.tok = np.zeros((rows, Tmax), np.int32)
        self.tok[:, 0] = bos
        self.score = np.zeros((rows, Tmax), np.float32)
        self.anc = np.repeat(np.arange(rows, dtype=np.int32)[:, None], Tmax, 1)
        self.ignore = np.zeros(rows, bool)
        self.parent = np.arange(rows, dtype=np.int32)
        self.rec_tok = np.zeros((rows, max_len + 1), np.int32)
        self.rec_pos = np.zeros((rows, max_len + 1), np.float32)
        self.rec_score = np.zeros(rows, np.float32)
        self.rec_len = np.zeros(rows, np.int32)
        self.n_hyp = np.zeros(n_sent, np.int32)
        self.sent_done = np.zeros(n_sent, np.int32)
        self.n_finished = 0
        self.min_gap = np.inf          # smallest difference of neighbouring finite scores among ranks 1 .. 2 * beam + 1 seen so far

    # ---- step 2 ----
    def rules(self, lp, step=None):
        step = self.counter if step is None else step
        lp = np.array(lp, np.float32, copy=True)[:, :self.V]
        if step < self.min_len and "eos_below_min_len" not in self.faults:
            lp[:, self.eos] = NEG
        lp[lp != lp] = NEG
        lp[:, self.pad] = NEG
        lp[:, self.unk] -= self.unk_penalty
        lp[:, self.never] = NEG
        if step >= self.max_len:
            keep = lp[:, self.eos].copy()
            lp[:] = NEG
            lp[:, self.eos] = keep
        return lp

    def history(self, r, upto):
        """(tokens, cumulative scores) of hypothesis row r at positions 0 .. upto through the ancestry table."""
        j = np.arange(upto + 1)
        a = self.anc[r, j]
        return self.tok[a, j], self.score[a, j]

    # ---- steps 3-6 ----
    def step(self, lp, ruled=False):
        step = self.counter
        if step > self.max_len:
            return
        lp = np.array(lp, np.float32)[:, :self.V] if ruled else self.rules(lp)
        beam, V, K = self.beam, self.V, 2 * self.beam
        for s in range(self.n_sent):
            r0 = s * beam
            if step == 0 and "step0_all_beams" not in self.faults:
                cand = lp[r0:r0 + 1].reshape(-1)
            elif step == 0:
                cand = lp[r0:r0 + beam].reshape(-1)
            else:
                cand = (lp[r0:r0 + beam] + self.score[r0:r0 + beam, step][:, None]).astype(np.float32).reshape(-1)
            cand = cand + np.float32(0)                                       # (-0 counts as +0)
            if "tie_higher_index_first" in self.faults:
                order = (len(cand) - 1 - np.argsort(-cand[::-1], kind="stable"))
            else:
                order = np.argsort(-cand, kind="stable")                      # the tie rule: equal scores keep flat-index order
            top = order[:K + 1]
            sc_sorted = cand[top]
            fin_sorted = sc_sorted[np.isfinite(sc_sorted)]
            if len(fin_sorted) > 1:
                self.min_gap = min(self.min_gap, float(np.min(fin_sorted[:-1] - fin_sorted[1:])))
            top = top[:K]
            c_score, c_tok, c_beam = cand[top], (top % V).astype(np.int32), (top // V).astype(np.int32)
            fin = (c_tok == self.eos) & (c_score != NEG)
            ign = self.ignore[r0:r0 + beam].copy()
            done = bool(self.sent_done[s]) and "finished_sentence_leaks" not in self.faults
            for i in range(beam):
                ok = fin[i] and (not ign[i] or "ignored_slot_finalised" in self.faults)
                if ok and not done and self.n_hyp[s] < beam:
                    self._finalise(s, r0 + c_beam[i], c_score[i], step)
            if not done:
                if self.n_hyp[s] == beam or step == self.max_len:
                    self.sent_done[s] = 1
                    self.n_finished += 1
            masked = fin.copy()
            masked[:beam] |= ign
            if step < self.max_len:
                cont = [i for i in range(K) if not masked[i]] + [i for i in range(K) if masked[i]]
                for k, i in enumerate(cont[:beam]):
                    r = r0 + k
                    self.tok[r, step + 1] = c_tok[i]
                    self.score[r, step + 1] = c_score[i]
                    self.parent[r] = r0 + c_beam[i]
                    self.ignore[r] = masked[i]
        self.counter = step + 1

    def _finalise(self, s, p, eos_score, step):
        h = s * self.beam + self.n_hyp[s]
        toks, cum = self.history(p, step)
        self.rec_tok[h, :step] = toks[1:]
        self.rec_tok[h, step] = self.eos
        c = np.concatenate([cum[1:], [eos_score]]).astype(np.float32)
        pos = c.copy()
        pos[1:] = c[1:] - c[:-1]
        self.rec_pos[h, :step + 1] = pos
        div = np.float32(float(step if "normalise_by_step" in self.faults else step + 1) ** self.len_penalty)
        with np.errstate(divide="ignore"):
            self.rec_score[h] = np.float32(eos_score) / div if self.normalize_scores else np.float32(eos_score)
        self.rec_len[h] = step + 1
        self.n_hyp[s] += 1

    def reorder(self):
        """The ancestry reorder behind step(): anc[r, j] = anc[parent[r], j] for j < counter (none past max_len)."""
        t = self.counter
        if t < 1 or t > self.max_len:
            return
        self.anc[:, :t] = self.anc[self.parent, :t]

    def hypotheses(self):
        """The records as generate() returns them: per sentence the hypotheses best first."""
        out = []
        for s in range(self.n_sent):
            hyps = []
            for k in range(int(self.n_hyp[s])):
                h, n = s * self.beam + k, int(self.rec_len[s * self.beam + k])
                hyps.append({"tokens": self.rec_tok[h, :n].astype(np.int64), "score": self.rec_score[h],
                             "positional_scores": self.rec_pos[h, :n].copy()})
            order = sorted(range(len(hyps)), key=lambda i: -float(hyps[i]["score"]))
            out.append([hyps[i] for i in order])
        return out
