"""fp64 restatement of the contract of st5_beam_cross_attn (csrc/beam_decode.hip) and of the host bookkeeping of beam search over a
slot cache (TransformerDecoder.init_beam_slots / reorder_beam_slots).  TEST INFRASTRUCTURE, plain torch / numpy on the CPU.

beam_cross_attn_ref: the cross-attention of multihead_attention.py:340-389 with one query per hypothesis row; row r belongs to live
sentence r // beam and reads the K|V block of original sentence sent[r // beam], stored once per sentence; a set padding byte excludes
a key (probability exactly 0); a sent entry outside [0, n_sent) gives NaN in that sentence's rows (context and record).
`fault` plants one of the mistakes the comparison against the brute-force form must catch.
reorder_ref / SlotSim: the ancestry table of st5_lm_reorder and a row-by-row simulation of what every hypothesis has written."""
import numpy as np
import torch

FAULTS = ("row_mod_beam", "sent_ignored", "v_offset_dropped", "padded_key_included", "record_wrong_sum")


def beam_cross_attn_ref(q, kv, k_off, sent, n_sent, beam, S, H, hd=64, kpm=None, fault=None):
    """q [rows, >= C]; kv [n_sent * S, ld]; sent int [n_live]; kpm bool / uint8 [n_sent, S] or None.
    Returns (ctx [rows, C], probs [rows, H, S]) in fp64."""
    assert fault is None or fault in FAULTS
    C = H * hd
    rows = q.shape[0]
    n_live = len(sent)
    assert rows == n_live * beam
    q = q.double()[:, :C]
    kv = kv.double()
    ctx = torch.empty(rows, C, dtype=torch.float64)
    probs = torch.empty(rows, H, S, dtype=torch.float64)
    for r in range(rows):
        live = r % beam if fault == "row_mod_beam" else r // beam
        live = min(live, n_live - 1)
        s = live if fault == "sent_ignored" else int(sent[live])
        if s < 0 or s >= n_sent:
            ctx[r] = float("nan")
            probs[r] = float("nan")
            continue
        blk = kv[s * S:(s + 1) * S]
        k = blk[:, k_off:k_off + C].view(S, H, hd)
        voff = k_off if fault == "v_offset_dropped" else k_off + C
        v = blk[:, voff:voff + C].view(S, H, hd)
        sc = torch.einsum("hd,jhd->hj", q[r].view(H, hd), k) * hd ** -0.5          # [H, S]
        ex = torch.zeros(S, dtype=torch.bool) if kpm is None or fault == "padded_key_included" else kpm[s].bool()
        sc = sc.masked_fill(ex.unsqueeze(0), float("-inf"))
        mx = sc.max(dim=1, keepdim=True)[0]
        e = torch.exp(sc - mx)                                                    # exp(-inf) = 0 exactly at an excluded key
        p = e / e.sum(dim=1, keepdim=True)
        ctx[r] = torch.einsum("hj,jhd->hd", p, v).reshape(C)
        probs[r] = e / (e.sum(dim=1, keepdim=True) + 1.0) if fault == "record_wrong_sum" else p
    return ctx, probs


def beam_cross_attn_brute(q, kv, k_off, sent, n_sent, beam, S, H, hd=64, kpm=None):
    """The same result the way the concatenating path gets it: K|V replicated per hypothesis row, one batched masked softmax."""
    C = H * hd
    rows = q.shape[0]
    row_sent = torch.as_tensor(np.asarray(sent), dtype=torch.long).repeat_interleave(beam)
    rep = kv.double().view(n_sent, S, -1)[row_sent]                               # [rows, S, ld]: beam copies per sentence
    k = rep[..., k_off:k_off + C].view(rows, S, H, hd).permute(0, 2, 1, 3)
    v = rep[..., k_off + C:k_off + 2 * C].view(rows, S, H, hd).permute(0, 2, 1, 3)
    sc = (q.double()[:, :C].view(rows, H, 1, hd) @ k.transpose(-1, -2)) * hd ** -0.5   # [rows, H, 1, S]
    if kpm is not None:
        sc = sc.masked_fill(kpm.bool()[row_sent].view(rows, 1, 1, S), float("-inf"))
    p = torch.softmax(sc, dim=-1)
    return (p @ v).reshape(rows, C), p.view(rows, H, S)


def reorder_ref(anc, order, t):
    """st5_lm_reorder: out[r, j] = anc[order[r], j] for j < t, = r from t on."""
    anc, order = np.asarray(anc), np.asarray(order)
    out = np.repeat(np.arange(len(order), dtype=np.int32)[:, None], anc.shape[1], axis=1)
    out[:, :t] = anc[order, :t]
    return out


class SlotSim:
    """Row-by-row simulation of beam search over a slot cache: `slots[r][j]` is what row r wrote at position j (a unique id, written
    once); every hypothesis carries the list of ids of its own history, copied on a reorder the way the concatenating cache is."""

    def __init__(self, n_sent, beam, Tmax):
        self.beam, self.Tmax = beam, Tmax
        self.slots = -np.ones((n_sent * beam, Tmax), dtype=np.int64)
        self.hist = [[] for _ in range(n_sent * beam)]
        self.sent = [s for s in range(n_sent) for _ in range(beam)]       # original sentence of every row
        self.t = 0

    def step(self):
        """every live row writes position t into its own slot row"""
        for r in range(len(self.hist)):
            uid = self.t * 100000 + r
            assert self.slots[r, self.t] == -1, "a slot is written once"
            self.slots[r, self.t] = uid
            self.hist[r] = self.hist[r] + [uid]
        self.t += 1

    def reorder(self, order):
        self.hist = [list(self.hist[o]) for o in order]
        self.sent = [self.sent[o] for o in order]

    def check(self, anc, sent_map):
        anc = np.asarray(anc)
        assert anc.shape[0] == len(self.hist)
        for r, h in enumerate(self.hist):
            got = [int(self.slots[anc[r, j], j]) for j in range(self.t)]
            assert got == h, (r, got, h)
            assert (anc[r, self.t:] == r).all(), r
            assert int(sent_map[r // self.beam]) == self.sent[r], (r, sent_map, self.sent)


def synthetic_sequence(n_sent, beam, steps, seed, drops):
    """A seeded beam-search trajectory: per step (order [n_live * beam] over the rows BEFORE the shrink, batch_idxs or None).  `drops`:
    {step: live sentences that leave after it}.  Parents are drawn inside the sentence, with repeats."""
    rng = np.random.RandomState(seed)
    live = n_sent
    out = []
    for step in range(steps):
        keep = [s for s in range(live) if s not in drops.get(step, ())]
        order = np.concatenate([s * beam + rng.randint(0, beam, size=beam) for s in keep]).astype(np.int64)
        out.append((order, np.asarray(keep, dtype=np.int64) if len(keep) != live else None))
        live = len(keep)
    return out
