"""numpy restatement of the per-sentence beam step of a beam-search stream (include/speecht5_hip.h: st5_beam_step_sents,
st5_beam_reorder_sents, st5_beam_sents_admit; speecht5_amd/beam_stream.py) on top of tests/beam_step_reference.py, and a host
simulation of the whole stream over tests/fake_seq_model.py.  TEST INFRASTRUCTURE: tests/test_beam_stream_cpu.py holds it to the
existing generator and to tts_stream.stream_schedule, tests/test_beam_stream_kernels_gpu.py holds the kernels to it.

State per slot: pos (steps done by the occupant), maxlen (its step limit), done (1 = finished or idle; every slot starts idle), moved
(1 = the last step advanced the slot), pos_rows[r] = pos[r // beam].  A step of slot s IS BeamStepRef.step of a one-sentence search at
counter pos[s] with max_len maxlen[s], on the slot's slices of the arrays; a done slot is not touched.

`faults`: names of planted faults, each a way the stream can be wrong (test_beam_stream_cpu.py shows that every one is caught)."""
import collections

import numpy as np

from tests.beam_step_reference import BeamStepRef

FAULTS = ("done_slot_advances", "reorder_unmoved", "admit_keeps_ignore", "admit_keeps_n_hyp")


class BeamStreamRef:
    def __init__(self, n_slots, beam, V, cap, S=1, *, faults=(), **rules):
        assert all(f in FAULTS for f in faults)
        self.n_slots, self.beam, self.V, self.cap, self.S = n_slots, beam, V, cap, S
        self.faults = set(faults)
        self.full = BeamStepRef(n_slots, beam, V, cap, 0, **rules)       # the arrays: rows = n_slots * beam, Tmax = cap + 2
        self.full.tok[:, 0] = 0
        self.rows, self.Tmax = self.full.rows, self.full.Tmax
        self.pos = np.zeros(n_slots, np.int32)
        self.maxlen = np.zeros(n_slots, np.int32)
        self.done = np.ones(n_slots, np.int32)
        self.moved = np.zeros(n_slots, np.int32)
        self.pos_rows = np.zeros(self.rows, np.int32)
        self.kpm = np.zeros((n_slots, S), np.uint8)
        self.min_gap = np.inf

    # the arrays under the kernel's names
    def __getattr__(self, name):
        if name in ("tok", "score", "anc", "ignore", "parent", "rec_tok", "rec_pos", "rec_score", "rec_len", "n_hyp"):
            return getattr(self.full, name)
        raise AttributeError(name)

    def _view(self, s):
        """A one-sentence BeamStepRef over slot s's slices (views: what it writes lands in the stream's arrays), at the slot's step."""
        f, b0, b1 = self.full, s * self.beam, (s + 1) * self.beam
        v = BeamStepRef.__new__(BeamStepRef)
        v.__dict__.update({k: getattr(f, k) for k in ("beam", "V", "pad", "unk", "eos", "unk_penalty", "min_len", "normalize_scores",
                                                      "len_penalty", "never", "faults", "Tmax")})
        v.n_sent, v.rows, v.max_len, v.counter = 1, self.beam, int(self.maxlen[s]), int(self.pos[s])
        v.tok, v.score, v.ignore = f.tok[b0:b1], f.score[b0:b1], f.ignore[b0:b1]
        v.anc = f.anc[b0:b1] - b0                      # (a copy with slot-local row indices: a step reads it and never writes it)
        v.parent = np.zeros(self.beam, np.int32)
        v.rec_tok, v.rec_pos, v.rec_score, v.rec_len = f.rec_tok[b0:b1], f.rec_pos[b0:b1], f.rec_score[b0:b1], f.rec_len[b0:b1]
        v.n_hyp, v.sent_done = f.n_hyp[s:s + 1], self.done[s:s + 1]
        v.n_finished, v.min_gap = 0, np.inf
        return v

    def rules(self, lp, s):
        """Slot s's ruled log-probabilities at its own step and limit (lp: the slot's [beam, V] rows)."""
        return self._view(s).rules(lp)

    def live(self, s):
        return not self.done[s] and 0 <= self.pos[s] <= self.maxlen[s]

    def step(self, lp, ruled=False):
        """lp [rows, >= V]: the rows of done slots are never read."""
        for s in range(self.n_slots):
            b0, b1 = s * self.beam, (s + 1) * self.beam
            runs = self.live(s) or ("done_slot_advances" in self.faults and 0 <= self.pos[s] <= self.maxlen[s])
            if not runs:
                self.moved[s] = 0
                continue
            v = self._view(s)
            if "done_slot_advances" in self.faults:
                v.sent_done = np.zeros(1, np.int32)
            written = v.counter < v.max_len
            v.step(np.asarray(lp)[b0:b1], ruled=ruled)
            if written:
                self.full.parent[b0:b1] = v.parent + b0
            if "done_slot_advances" in self.faults and v.sent_done[0]:
                self.done[s] = 1
            self.min_gap = min(self.min_gap, v.min_gap)
            self.pos[s] += 1
            self.pos_rows[b0:b1] = self.pos[s]
            self.moved[s] = 1

    def reorder(self):
        f = self.full
        for s in range(self.n_slots):
            if not self.moved[s] and "reorder_unmoved" not in self.faults:
                continue
            t = int(self.pos[s])
            if t < 1 or t > self.maxlen[s]:
                continue
            b0, b1 = s * self.beam, (s + 1) * self.beam
            f.anc[b0:b1, :t] = f.anc[f.parent[b0:b1], :t]

    def admit(self, slot, max_len, frames, bos):
        if not 0 <= slot < self.n_slots:
            return
        f, b0, b1 = self.full, slot * self.beam, (slot + 1) * self.beam
        f.anc[b0:b1] = np.arange(b0, b1, dtype=np.int32)[:, None]
        f.tok[b0:b1, 0] = bos
        f.score[b0:b1, 0] = 0
        if "admit_keeps_ignore" not in self.faults:
            f.ignore[b0:b1] = False
        f.rec_len[b0:b1] = 0
        if "admit_keeps_n_hyp" not in self.faults:
            f.n_hyp[slot] = 0
        self.pos[slot] = 0
        self.pos_rows[b0:b1] = 0
        self.maxlen[slot] = min(max(int(max_len), 0), self.cap)
        self.done[slot] = 0
        fr = min(max(int(frames), 0), self.S)
        self.kpm[slot] = np.arange(self.S) >= fr

    def history(self, r, upto):
        return self.full.history(r, upto)

    def hypotheses(self, s):
        """Slot s's record as generate() returns a sentence: the hypotheses best first."""
        f, hyps = self.full, []
        for k in range(int(f.n_hyp[s])):
            h = s * self.beam + k
            n = int(f.rec_len[h])
            hyps.append({"tokens": f.rec_tok[h, :n].astype(np.int64), "score": f.rec_score[h].copy(),
                         "positional_scores": f.rec_pos[h, :n].copy()})
        order = sorted(range(len(hyps)), key=lambda i: -float(hyps[i]["score"]))
        return [hyps[i] for i in order]


def never_of(gen):
    never = np.zeros(gen.vocab_size, bool)
    never[gen.blank] = True
    if gen.mask != gen.unk:
        never[gen.mask] = True
    never[gen.mask_idxs.numpy()] = True
    return never


def simulate_stream(gen, requests, n_slots, max_src_len, poll_steps, faults=()):
    """The loop of beam_stream.BeamStream on the host: requests [(key, source [n], max_len or None)] through n_slots slots of the
    restatement, the fake model as the decoder (each live slot's rows decoded from their own prefixes against the request encoded
    ALONE).  Returns ([(key, hyps)] in completion order, ticks, polls, {key: steps})."""
    import torch
    from speecht5_amd.tts_stream import assign_rows
    beam = gen.beam_size
    limit = lambda n, ml: int(ml) if ml is not None else min(int(gen.max_len_a * n + gen.max_len_b), gen.max_len - 1)   # noqa: E731
    cap = limit(max_src_len, None)
    ref = BeamStreamRef(n_slots, beam, gen.vocab_size, cap, faults=faults, pad=gen.pad, unk=gen.unk, eos=gen.eos,
                        unk_penalty=gen.unk_penalty, min_len=gen.min_len, normalize_scores=gen.normalize_scores,
                        len_penalty=gen.len_penalty, never=never_of(gen))
    waiting = collections.deque()
    for key, src, ml in requests:
        assert src.numel() <= max_src_len and limit(src.numel(), ml) <= cap
        net = {"source": src.unsqueeze(0), "padding_mask": torch.zeros(1, src.numel(), dtype=torch.bool)}
        enc = gen.model.forward_encoder(net)
        waiting.append((key, gen.model.reorder_encoder_out(enc, torch.zeros(beam, dtype=torch.long)), limit(src.numel(), ml)))
    occupant, out, steps = [None] * n_slots, [], {}
    ticks = polls = 0
    inflight = False
    while True:
        if inflight:
            polls += 1
            for s in range(n_slots):
                if occupant[s] is not None and ref.done[s]:
                    out.append((occupant[s][0], ref.hypotheses(s)))
                    steps[occupant[s][0]] = int(ref.pos[s])
                    occupant[s] = None
        pairs = assign_rows([s for s in range(n_slots) if occupant[s] is None], len(waiting))
        if not pairs and all(o is None for o in occupant):
            break
        for s, _ in pairs:
            occupant[s] = waiting.popleft()
            ref.admit(s, occupant[s][2], 1, gen.eos)
        for _ in range(poll_steps):
            lp = np.zeros((ref.rows, gen.vocab_size), np.float32)
            for s in range(n_slots):
                if occupant[s] is None or not (ref.live(s) or "done_slot_advances" in faults):
                    continue
                t = min(int(ref.pos[s]), ref.Tmax - 1)
                toks = np.stack([ref.history(r, t)[0] for r in range(s * beam, (s + 1) * beam)]).astype(np.int64)
                lprobs, _ = gen.model.forward_decoder(torch.from_numpy(toks), occupant[s][1], [{}], gen.temperature)
                lp[s * beam:(s + 1) * beam] = lprobs.numpy()
            ref.step(lp)
            ref.reorder()
            ticks += 1
        inflight = True
    return out, ticks, polls, steps, ref
