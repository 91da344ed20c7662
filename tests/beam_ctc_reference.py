"""numpy restatement of the CTC part of a device-stepped beam search step (csrc/beam_ctc.hip, include/speecht5_hip.h): the candidate
pick under the TIE RULE (higher value first, among equal values the lower token; never-tokens and NaN count as -inf), the fp32 mix
of attention and CTC scores, and the select with its `unknown` rule.  The prefix scores themselves are not restated: they come from
tests/ctc_rows_reference.py (CPU tests) or from the existing rows entries (GPU tests).  TEST INFRASTRUCTURE.

`faults`: names of planted faults, each a way the step can be wrong (tests/test_beam_ctc_cpu.py shows that every one is caught by
the comparisons tests/test_beam_ctc_gpu.py makes)."""
import numpy as np

from tests.ctc_reference import LOGZERO

FAULTS = ("weights_swapped", "prev_not_subtracted", "state_from_own_row", "unknown_from_ignored_row", "tie_higher_token_first",
          "never_not_masked")
NEG = np.float32(-np.inf)


def candidates(lp, never, nc, faults=()):
    """int32 [rows, nc]: the nc best tokens of every row of lp [rows, V] in rank order."""
    lp = np.array(lp, np.float32)
    v = lp.copy()
    v[v != v] = NEG
    if "never_not_masked" not in faults:
        v[:, np.asarray(never).astype(bool)] = NEG
    v = v + np.float32(0)                                                     # (-0 counts as +0)
    out = np.empty((lp.shape[0], nc), np.int32)
    for r in range(lp.shape[0]):
        if "tie_higher_token_first" in faults:
            order = len(v[r]) - 1 - np.argsort(-v[r, ::-1], kind="stable")
        else:
            order = np.argsort(-v[r], kind="stable")                          # the tie rule: equal values keep token order
        out[r] = order[:nc]
    return out


def mix(lp, cs, log_psi, prev, w, faults=()):
    """lp with lp[r, cs[r, j]] = (float)(1 - w) * lp + (float)w * (log_psi[r, j] - prev[r]), every operation rounded to fp32."""
    lp = np.array(lp, np.float32)
    wa, wb = np.float32(1 - w), np.float32(w)
    if "weights_swapped" in faults:
        wa, wb = wb, wa
    rows = np.arange(lp.shape[0])[:, None]
    d = np.asarray(log_psi, np.float32) - (np.float32(0) if "prev_not_subtracted" in faults else np.asarray(prev, np.float32)[:, None])
    with np.errstate(invalid="ignore"):
        lp[rows, cs] = (wa * lp[rows, cs]).astype(np.float32) + (wb * d.astype(np.float32)).astype(np.float32)
    return lp


def select(parent, token, cs, log_psi, r_new, lens, beam, ignore, sent_done, faults=()):
    """The continued rows' prefix state: (state [rows, Tfr, 2], prev [rows], unknown).  r_new [rows, Tfr, nc, 2] (frames at and
    behind a sentence's count are not read), token [rows] the token each row was continued by, parent [rows] the row it continues."""
    rows, Tfr = r_new.shape[:2]
    state = np.full((rows, Tfr, 2), LOGZERO, np.float32)
    prev = np.zeros(rows, np.float32)
    unknown = 0
    for r in range(rows):
        p = r if "state_from_own_row" in faults else int(parent[r])
        s = r // beam
        hit = np.nonzero(cs[p] == token[r])[0]
        slot = int(hit[0]) if len(hit) else 0
        T = int(lens[s])
        state[r, :T] = r_new[p, :T, slot]
        prev[r] = log_psi[p, slot]
        counts = not sent_done[s] and (not ignore[r] or "unknown_from_ignored_row" in faults)
        if not len(hit) and counts:
            unknown = 1
    return state, prev, unknown
