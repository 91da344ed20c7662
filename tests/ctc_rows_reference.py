"""Plain reference of the rows form of the CTC prefix scorer (csrc/ctc_prefix.hip, the st5_ctc_*_rows entries): a batch of
posteriors x [S, Tmax, V] right-padded in time, sentence s scored on its own frames x[s, :T_s] with tests/ctc_reference.py's
prefix_initial / prefix_score, which this module imports and does not restate.  float32 restates the kernels' arithmetic,
float64 is the reference.

What the single-posterior recursion does not define is a prefix with more labels than its sentence has frames (out_len > T_s; in
a batch a short sentence meets it while the others decode on).  No alignment of T_s frames emits more than T_s labels, so every
label extension has probability zero; the prefix ending here has the prefix's own probability logaddexp(r_prev[T_s - 1]) (zero
too, when the state came from this recursion); the extensions' states are all zero.  Written out in rows_score below."""
import numpy as np

from tests.ctc_reference import LOGZERO, prefix_initial, prefix_score


def rows_initial(x, lens, blank, dtype=np.float64):
    """r [S, Tmax, 2]: prefix_initial of x[s, :T_s] in its first T_s frames, LOGZERO behind."""
    x = np.asarray(x)
    S, Tmax, _ = x.shape
    r = np.full((S, Tmax, 2), LOGZERO, dtype=dtype)
    for s in range(S):
        r[s, :lens[s]] = prefix_initial(x[s, :lens[s]], blank, dtype)
    return r


def rows_score(x, lens, sent, last, out_len, cs, r_prev, blank, eos, dtype=np.float64):
    """x [S, Tmax, V], lens [S], sent [nh] the sentence of each hypothesis row, last [nh], cs [nh, nc], r_prev [nh, Tmax, 2].
    Returns log_psi [nh, nc] and r [nh, nc, Tmax, 2] (LOGZERO behind each row's frames)."""
    x, cs, last, r_prev = np.asarray(x), np.asarray(cs), np.asarray(last), np.asarray(r_prev)
    nh, nc = cs.shape
    Tmax = x.shape[1]
    lz = np.asarray(LOGZERO, dtype=dtype)
    log_psi = np.full((nh, nc), lz, dtype=dtype)
    r = np.full((nh, nc, Tmax, 2), lz, dtype=dtype)
    for h in range(nh):
        T = int(lens[sent[h]])
        if out_len > T:                                            # more labels than frames
            rp = r_prev[h, T - 1].astype(dtype)
            log_psi[h] = np.where(cs[h] == eos, np.logaddexp(rp[0], rp[1]), lz)
            log_psi[h] = np.where(cs[h] == blank, lz, log_psi[h])
            continue
        p, rr = prefix_score(x[sent[h], :T], last[h:h + 1], out_len, cs[h:h + 1], r_prev[h:h + 1, :T], blank, eos, dtype)
        log_psi[h], r[h, :, :T] = p[0], rr[0]
    return log_psi, r
