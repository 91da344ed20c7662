"""numpy restatement of the finite-gradient guard of the Adam step (st5_adam_step_guard, include/speecht5_hip.h): the
verdict from a squared norm, the guard block's cells, the applied-step count and Adam in fp32 with the kernel's formula.

guard_launch() is the protocol as the kernel runs it (cells read and written by parity of the step); specification() is what it has to
amount to, written without any cell: the non-finite updates are dropped from the sequence and plain Adam runs over the rest with the
steps renumbered 1, 2, ...  tests/test_nonfinite_guard_cpu.py sweeps the first against the second and checks that the sweep tells every
planted fault (FAULTS) from the protocol."""
import numpy as np

GUARD_COUNT, GUARD_SKIPPED, GUARD_STEP, GUARD_CELLS = 0, 2, 3, 4      # ST5_GUARD_*
F = np.float32
FLT_MAX = np.finfo(np.float32).max

FAULTS = (
    "wrong_parity",           # reads the cell of parity t & 1, writes the other one
    "count_from_own_cell",    # the publisher adds this launch's verdict to the cell it writes instead of the cell everybody read
    "publish_only_on_skip",   # a finite step does not carry the count over to its parity's cell
    "bias_from_t",            # bias corrections from the attempted step count
    "verdict_misses_nan",     # x > FLT_MAX instead of !(x <= FLT_MAX)
    "verdict_misses_overflow",  # isnan(x) alone
    "skip_decays_weights",    # a skipped step still applies p *= 1 - lr * wd
    "skip_keeps_gradient",    # a skipped step leaves the non-finite gradient behind
)


def sumsq(g, g2=None):
    """fp32 sum of squares the way it can overflow: every product and partial sum rounded to fp32 (the kernel's partition differs;
    only finiteness matters here)."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = g.astype(F) if g2 is None else (g.astype(F) + g2.astype(F))
        return F(np.sum(x * x, dtype=F))


def skip_verdict(gnorm_sq, fault=None):
    x = F(gnorm_sq)
    if fault == "verdict_misses_nan":
        return bool(x > FLT_MAX)
    if fault == "verdict_misses_overflow":
        return bool(np.isnan(x))
    return not bool(x <= FLT_MAX)


def adam_apply(p, g, m, v, *, lr, b1, b2, eps, wd, t, gnorm_sq, max_norm, gscale):
    """adam_kernel's expressions in fp32 (csrc/optim.hip); returns new (p, m, v)."""
    lr, b1, b2, eps, wd, t, gscale, max_norm = map(F, (lr, b1, b2, eps, wd, t, gscale, max_norm))
    bc1, bc2 = F(1) - np.power(b1, t, dtype=F), F(1) - np.power(b2, t, dtype=F)
    coef = gscale
    if max_norm > 0:
        norm = np.sqrt(F(gnorm_sq)) * gscale
        c = max_norm / (norm + F(1e-6))
        coef = coef * (c if c < 1 else F(1))
    step = lr * np.sqrt(bc2) / bc1
    ge = g.astype(F) * coef
    m = b1 * m + (F(1) - b1) * ge
    v = b2 * v + (F(1) - b2) * ge * ge
    p = p * (F(1) - lr * wd) - step * m / (np.sqrt(v) + eps)
    return p.astype(F), m.astype(F), v.astype(F)


def guard_launch(state, guard, t, g, hp, fault=None):
    """One launch of the guarded step at attempted step t (1, 2, ...: it advances by one per launch).  state = [p, m, v] (replaced in
    place), guard = int32[GUARD_CELLS], g = the gradient (zeroed in place, as with zero_grads).  Every reader's view is the value the
    cells had BEFORE the launch: reads and the publisher's writes touch different cells, which the sweep checks by construction --
    `before` is taken from a snapshot, so a protocol that needed a value written in this launch would not get it."""
    old = guard.copy()
    r, w = GUARD_COUNT + ((t & 1) ^ 1), GUARD_COUNT + (t & 1)
    if fault == "wrong_parity":
        r, w = w, r
    gsq = sumsq(g)
    skip = skip_verdict(gsq, fault)
    before = int(old[r])
    # the publisher (one thread)
    if fault == "count_from_own_cell":
        guard[w] = old[w] + int(skip)
    elif fault == "publish_only_on_skip":
        if skip:
            guard[w] = before + 1
    else:
        guard[w] = before + int(skip)
    guard[GUARD_SKIPPED] = int(skip)
    guard[GUARD_STEP] = t
    if skip:
        if fault == "skip_decays_weights":
            state[0] = (state[0] * (F(1) - F(hp["lr"]) * F(hp["wd"]))).astype(F)
        if fault != "skip_keeps_gradient":
            g[...] = 0
        return
    t_eff = t if fault == "bias_from_t" else t - before
    with np.errstate(over="ignore", invalid="ignore"):
        state[0], state[1], state[2] = adam_apply(state[0], g, state[1], state[2], t=t_eff, gnorm_sq=gsq, **hp)
    g[...] = 0


def skipped_count(guard):
    return int(guard[GUARD_COUNT + (int(guard[GUARD_STEP]) & 1)])


def specification(p0, grads, hp):
    """What a guarded run amounts to: the updates whose squared norm is not finite never happened (as far as p, m, v and Adam's step
    count go); returns (p, m, v, number of dropped updates, per-update verdicts)."""
    p, m, v = p0.astype(F), np.zeros_like(p0, dtype=F), np.zeros_like(p0, dtype=F)
    applied, verdicts = 0, []
    for g in grads:
        gsq = sumsq(g)
        bad = not np.isfinite(gsq)
        verdicts.append(int(bad))
        if bad:
            continue
        applied += 1
        p, m, v = adam_apply(p, g, m, v, t=applied, gnorm_sq=gsq, **hp)
    return p, m, v, len(grads) - applied, verdicts


def run_protocol(p0, grads, hp, fault=None):
    """The same sequence through guard_launch(); returns (p, m, v, count, per-update flags, gradients left behind all zero?)."""
    state = [p0.astype(F), np.zeros_like(p0, dtype=F), np.zeros_like(p0, dtype=F)]
    guard = np.zeros(GUARD_CELLS, dtype=np.int32)
    flags, clean = [], True
    for t, g in enumerate(grads, start=1):
        g = g.astype(F).copy()
        before = [x.copy() for x in state]
        guard_launch(state, guard, t, g, hp, fault)
        flags.append(int(guard[GUARD_SKIPPED]))
        clean = clean and not g.any() and not np.isnan(g).any()
        if flags[-1]:      # a skipped launch leaves the bytes of p, m, v as they were
            clean = clean and all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(before, state))
    return state[0], state[1], state[2], skipped_count(guard), flags, clean
