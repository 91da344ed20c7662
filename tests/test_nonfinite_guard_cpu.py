"""CPU: the finite-gradient guard's protocol (tests/nonfinite_reference.py) against its specification -- non-finite updates dropped,
plain Adam over the rest with the steps renumbered -- over every verdict sequence of up to five updates and three kinds of bad
gradient; every planted fault is told apart by the same sweep.  Also: the guard block's layout is one set of numbers in the header, the
Python constants and the restatement, and the signature table knows the entry point."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import nonfinite_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = dict(lr=1e-2, b1=0.9, b2=0.98, eps=1e-6, wd=0.01, max_norm=1.0, gscale=0.5)
N = 7


def _grads(verdicts, seed=0):
    """One gradient per update; a bad one is, in turn, a single +inf, a single NaN, and all-finite 1e20 (squares overflow fp32)."""
    rng = np.random.default_rng(seed)
    out, kind = [], 0
    for bad in verdicts:
        g = rng.standard_normal(N).astype(np.float32)
        if bad:
            if kind % 3 == 0:
                g[3] = np.inf
            elif kind % 3 == 1:
                g[N - 1] = np.nan
            else:
                g[:] = 1e20
            kind += 1
        out.append(g)
    return out


def _sequences():
    seqs = [s for n in range(1, 6) for s in itertools.product((0, 1), repeat=n)]
    seqs += [(1, 0, 0, 0, 0, 0), (0, 1, 1, 0, 0, 0), (0, 0, 0, 0, 0, 1), (1, 1, 1, 0, 1, 0, 0), (0, 0, 1, 0, 0, 0)]
    return seqs


def _agrees(seq, fault=None):
    p0 = np.linspace(-1, 1, N).astype(np.float32)
    grads = _grads(seq)
    want = R.specification(p0, grads, HP)
    got = R.run_protocol(p0, grads, HP, fault)
    same = all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(want[:3], got[:3]))
    return same and want[3] == got[3] and want[4] == got[4] and got[5]


def test_verdict():
    f32 = np.float32
    for x in (0.0, 1.0, np.finfo(f32).max, np.finfo(f32).tiny):
        assert not R.skip_verdict(f32(x))
    for x in (np.inf, np.nan, -np.nan):
        assert R.skip_verdict(f32(x))
    assert R.skip_verdict(R.sumsq(np.full(4, 1e20, dtype=f32)))          # finite elements, overflowed sum
    assert R.skip_verdict(R.sumsq(np.array([np.inf], f32), np.array([-np.inf], f32)))      # the pair form: inf - inf is NaN
    assert not R.skip_verdict(R.sumsq(np.full(4, 1e18, dtype=f32)))


def test_protocol_equals_specification_over_all_sequences():
    seqs = _sequences()
    assert (1, 0) in seqs and (0, 1, 1) in seqs and (0, 0, 1) in seqs    # a skip first, two in a row, a skip last
    for seq in seqs:
        assert _agrees(seq), seq


def test_applied_steps_are_renumbered():
    """After one skip at step 2, step 3 is Adam's SECOND step: same bits as the unguarded formula at t = 2."""
    p0 = np.linspace(-1, 1, N).astype(np.float32)
    grads = _grads((0, 1, 0))
    p, m, v, count, flags, clean = R.run_protocol(p0, grads, HP)
    q, qm, qv = R.adam_apply(p0, grads[0], np.zeros(N, np.float32), np.zeros(N, np.float32), t=1, gnorm_sq=R.sumsq(grads[0]), **HP)
    q, qm, qv = R.adam_apply(q, grads[2], qm, qv, t=2, gnorm_sq=R.sumsq(grads[2]), **HP)
    assert count == 1 and flags == [0, 1, 0] and clean
    assert np.array_equal(p, q) and np.array_equal(m, qm) and np.array_equal(v, qv) and np.isfinite(p).all()


@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_sweep_catches_a_planted_fault(fault):
    caught = [seq for seq in _sequences() if not _agrees(seq, fault)]
    assert caught, f"no verdict sequence tells the fault {fault!r} from the protocol"


def test_layout_is_the_same_everywhere():
    hdr = open(os.path.join(ROOT, "include", "speecht5_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (ST5_GUARD_[A-Z]+) (\d+)", hdr)}
    from speecht5_amd import ddp
    for name in ("COUNT", "SKIPPED", "STEP", "CELLS"):
        assert defs["ST5_GUARD_" + name] == getattr(ddp, "GUARD_" + name) == getattr(R, "GUARD_" + name), name
    # two count cells, then the flag, then the step, nothing overlapping
    assert sorted({defs["ST5_GUARD_COUNT"], defs["ST5_GUARD_COUNT"] + 1, defs["ST5_GUARD_SKIPPED"], defs["ST5_GUARD_STEP"]}) == list(range(defs["ST5_GUARD_CELLS"]))


def test_signature_table_has_the_entry_point():
    from speecht5_amd import hip
    assert "st5_adam_step_guard" in hip.exported_symbols()
    hdr = open(os.path.join(ROOT, "include", "speecht5_hip.h")).read()
    decl = re.search(r"int st5_adam_step_guard\(([^;]*)\);", hdr).group(1)
    pair = re.search(r"int st5_adam_step_pair\(([^;]*)\);", hdr).group(1)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]
    assert norm(decl) == norm(pair)[:-1] + ["int32_t* guard", "void* stream"]     # the pair form's arguments plus the guard block
