"""The finite-gradient guard of the Adam step on the GPU (st5_adam_step_guard, FusedAdam(skip_nonfinite=True),
PretrainUpdate(nonfinite="skip")).

Kernel level (fp32 buffers + bf16 mirror; 3 elements = tail only, 4099 = a few blocks of body + a three-element tail, 4 (4096 * 256 +
300) + 1 = more 16-byte vectors than the 4096-block grid holds: the grid-stride loop wraps; one buffer and the pair, by-value and
device hyper): a finite step is st5_adam_step_pair bit for bit; a non-finite norm -- one +inf, one NaN in the second buffer only,
finite 1e20s whose squares overflow -- leaves p, m, v and the mirror byte-equal to before and both gradient buffers zero; the finite
step after a skipped one at step t is the unguarded step t - 1.

Update level (the tiny pre-training pair and the construction of tests/test_batch_feed_gpu.py, six fed updates, the third batch's
speech micro-batch with one +inf planted in the mel target `dec_target`, which only the loss reads -- the forward, its activations and
the BatchNorm statistics stay finite; the Tacotron loss's backward turns it into NaN gradients of the post-net output, which
test_bad_batch_without_the_guard_poisons_the_parameters and the recorded gnorm confirm)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from speecht5_amd import functional as Fn
from tests.test_batch_feed_gpu import _pairs, _same
from tests.util import Task, load_golden, to_dev

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SIZES = [3, 4099, 4 * (4096 * 256 + 300) + 1]
HP = dict(lr=1e-3, b1=0.9, b2=0.98, eps=1e-6, wd=0.01, gscale=0.5)
ERR_ARG = 1


# ---- kernel level ------------------------------------------------------------------------------------------------------------------
class _Bufs:
    def __init__(self, n, dev, seed=0):
        g = torch.Generator(device=dev).manual_seed(seed + n % 1000)
        r = lambda: torch.randn(n, device=dev, generator=g)
        self.n = n
        self.p, self.g, self.g2, self.m = r(), r(), r(), r() * 0.1
        self.v = torch.rand(n, device=dev, generator=g) * 0.01
        self.mirror = self.p.to(BF)
        self.gn = torch.zeros(1, device=dev)

    def clone(self):
        o = object.__new__(_Bufs)
        o.n = self.n
        for k in ("p", "g", "g2", "m", "v", "mirror", "gn"):
            setattr(o, k, getattr(self, k).clone())
        return o

    def state(self):
        return [self.p, self.m, self.v, self.mirror]


def _step(b, step, *, pair, hyper, clip=1.0, guard=None):
    """sumsq + one Adam launch on the buffers `b` (the guarded entry point when `guard` is given); returns the squared norm."""
    from speecht5_amd import hip
    L = hip.lib()
    if pair:
        hip.check(L.st5_sumsq_pair(b.g.data_ptr(), b.g2.data_ptr(), b.gn.data_ptr(), b.n, 1.0, 0, hip.stream()), "st5_sumsq_pair")
    else:
        hip.check(L.st5_sumsq(b.g.data_ptr(), b.gn.data_ptr(), b.n, 1.0, 0, hip.F32, hip.stream()), "st5_sumsq")
    gsq = float(b.gn)
    # device hyper: the by-value lr / step are NOT what the kernel may use (lr 0 would leave p unchanged, step 0 is refused without hyper)
    hyp = torch.tensor([HP["lr"], float(step)], device=b.p.device) if hyper else None
    lr, st = (0.0, 0) if hyper else (HP["lr"], step)
    args = [b.p.data_ptr(), b.g.data_ptr(), b.g2.data_ptr() if pair else 0, 1, b.m.data_ptr(), b.v.data_ptr(), b.n, lr, HP["b1"], HP["b2"],
            HP["eps"], HP["wd"], st, b.gn.data_ptr(), clip, HP["gscale"], b.mirror.data_ptr(), hip.ptr(hyp)]
    if guard is not None:
        hip.check(L.st5_adam_step_guard(*args, guard.data_ptr(), hip.stream()), "st5_adam_step_guard")
    else:
        hip.check(L.st5_adam_step_pair(*args, hip.stream()), "st5_adam_step_pair")
    torch.cuda.synchronize()
    return gsq


def _guard(dev):
    from speecht5_amd.ddp import GUARD_CELLS
    return torch.zeros(GUARD_CELLS, dtype=torch.int32, device=dev)


def _cells(guard):
    from speecht5_amd.ddp import GUARD_COUNT, GUARD_SKIPPED, GUARD_STEP
    c = guard.tolist()
    return {"count": c[GUARD_COUNT + (c[GUARD_STEP] & 1)], "flag": c[GUARD_SKIPPED], "step": c[GUARD_STEP]}


def _assert_same(xs, ys, what):
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert _same(x, y), (what, i)


def _zero(t):
    return not bool(t.view(torch.int32).any())       # (exact +0.0 everywhere: no -0.0, no NaN)


@pytest.mark.parametrize("hyper", [False, True], ids=["by_value", "hyper"])
@pytest.mark.parametrize("pair", [False, True], ids=["one_buffer", "pair"])
@pytest.mark.parametrize("n", SIZES)
def test_finite_step_equals_the_unguarded_step(cuda, n, pair, hyper):
    a = _Bufs(n, cuda)
    b = a.clone()
    guard = _guard(cuda)
    _step(a, 1, pair=pair, hyper=hyper)
    gsq = _step(b, 1, pair=pair, hyper=hyper, guard=guard)
    assert np.isfinite(gsq)
    _assert_same(a.state(), b.state(), "finite step")
    assert not _same(a.p, _Bufs(n, cuda).p)                   # (the step did something)
    assert _same(a.g, b.g) and _same(a.g2, b.g2)              # the zeroed gradient buffers (the untouched g2 of the one-buffer form)
    assert _zero(b.g) and (_zero(b.g2) if pair else not _zero(b.g2))
    assert _cells(guard) == {"count": 0, "flag": 0, "step": 1}


def _plant(b, kind, pair):
    if kind == "inf":
        b.g[b.n // 2] = float("inf")
    elif kind == "nan_second":
        (b.g2 if pair else b.g)[b.n - 1] = float("nan")      # the pair form: in g2 ONLY (one buffer: there is no second one)
    else:
        b.g.fill_(1e20)                                      # every element finite, the squares overflow fp32
        assert bool(torch.isfinite(b.g).all())


@pytest.mark.parametrize("kind", ["inf", "nan_second", "overflow"])
@pytest.mark.parametrize("hyper", [False, True], ids=["by_value", "hyper"])
@pytest.mark.parametrize("pair", [False, True], ids=["one_buffer", "pair"])
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_step_is_skipped(cuda, n, pair, hyper, kind):
    b = _Bufs(n, cuda)
    _plant(b, kind, pair)
    before = b.clone()
    guard = _guard(cuda)
    gsq = _step(b, 1, pair=pair, hyper=hyper, guard=guard)
    assert not np.isfinite(gsq), gsq                          # the bad element reaches gnorm_sq[0] through the partial sums
    _assert_same(before.state(), b.state(), "skipped step")
    assert _zero(b.g) and (_zero(b.g2) if pair else _same(b.g2, before.g2))
    assert _cells(guard) == {"count": 1, "flag": 1, "step": 1}


@pytest.mark.parametrize("hyper", [False, True], ids=["by_value", "hyper"])
@pytest.mark.parametrize("pair", [False, True], ids=["one_buffer", "pair"])
def test_finite_step_after_a_skipped_one_is_the_unguarded_step_before(cuda, pair, hyper):
    """Steps 1 (finite), 2 (skipped), 3 and 4 (finite): the guarded run equals the unguarded steps 1, 2, 3 on the finite gradients."""
    n = 4099
    a = _Bufs(n, cuda)
    b = a.clone()
    guard = _guard(cuda)
    fresh = [(torch.randn(n, device=cuda), torch.randn(n, device=cuda)) for _ in range(4)]
    seen = []
    for t in (1, 2, 3, 4):
        b.g.copy_(fresh[t - 1][0]); b.g2.copy_(fresh[t - 1][1])
        if t == 2:
            b.g[7] = float("inf")
        _step(b, t, pair=pair, hyper=hyper, guard=guard)
        seen.append(_cells(guard))
    for t_ref, t in enumerate((1, 3, 4), start=1):
        a.g.copy_(fresh[t - 1][0]); a.g2.copy_(fresh[t - 1][1])
        _step(a, t_ref, pair=pair, hyper=hyper)
    assert seen == [{"count": 0, "flag": 0, "step": 1}, {"count": 1, "flag": 1, "step": 2}, {"count": 1, "flag": 0, "step": 3},
                    {"count": 1, "flag": 0, "step": 4}]
    _assert_same(a.state(), b.state(), "steps 1, [2], 3, 4 against 1, 2, 3")
    assert bool(torch.isfinite(b.p).all())


def test_argument_errors(cuda):
    from speecht5_amd import hip
    L = hip.lib()
    b = _Bufs(8, cuda)
    guard = _guard(cuda)
    before = b.clone()

    def call(gn, gd):
        return L.st5_adam_step_guard(b.p.data_ptr(), b.g.data_ptr(), 0, 1, b.m.data_ptr(), b.v.data_ptr(), b.n, 1e-3, 0.9, 0.98, 1e-6, 0.01, 1,
                                     gn, 1.0, 1.0, b.mirror.data_ptr(), 0, gd, hip.stream())
    assert call(b.gn.data_ptr(), 0) == ERR_ARG          # no guard block
    assert call(0, guard.data_ptr()) == ERR_ARG         # no norm: the guarded form has no meaning without one
    torch.cuda.synchronize()
    _assert_same(before.state() + [before.g], b.state() + [b.g], "refused call")
    assert guard.tolist() == [0, 0, 0, 0]


def test_fused_adam_without_clipping_still_skips(cuda):
    """FusedAdam(skip_nonfinite=True, clip_norm=0): the norm is computed although nothing clips; a finite step equals the unguarded,
    unclipped FusedAdam step, a non-finite one is skipped."""
    from speecht5_amd.ddp import FlatGradDataParallel, FusedAdam

    def run(guarded, bad_second):
        torch.manual_seed(3)
        model = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.Linear(17, 5)).to(cuda)
        ddp = FlatGradDataParallel(model, bucket_groups=[])
        try:
            opt = FusedAdam(ddp, lr=1e-2, clip_norm=0.0, weight_decay=0.01, **({"skip_nonfinite": True} if guarded else {}))
            g = torch.Generator(device=cuda).manual_seed(5)
            states = []
            for k in range(3):
                ddp.zero_grad()
                ddp.flat.copy_(torch.randn(ddp.flat.numel(), device=cuda, generator=g) * 30)      # (a norm any clip would act on)
                if bad_second and k == 1:
                    ddp.flat[11] = float("nan")
                opt.step(0.5)
                torch.cuda.synchronize()
                states.append((opt.pflat.clone(), opt.m.clone(), opt.v.clone()))
                assert _zero(ddp.flat)
            return states, (opt.skipped() if guarded else None)
        finally:
            ddp.close()
            Fn.weight_cache.clear()
            Fn.set_layer_boundary_hook(None)

    ref, _ = run(False, False)
    got, n = run(True, False)
    assert n == 0
    for r, s in zip(ref, got):
        _assert_same(r, s, "clip_norm = 0, finite")
    bad, n = run(True, True)
    assert n == 1
    _assert_same(bad[0], bad[1], "clip_norm = 0, the skipped second step")
    _assert_same(ref[0], bad[0], "the first step")
    assert not _same(bad[1][0], bad[2][0]) and bool(torch.isfinite(bad[2][0]).all())


# ---- update level ------------------------------------------------------------------------------------------------------------------
BAD = 3      # the update (1-based) that trains on the bad batch


def _source(cuda, bad):
    """Six pairs: the five of tests/test_batch_feed_gpu.py and the second one again; `bad`: the third pair's speech micro-batch with
    one +inf in the mel target (a copy: the shared pairs stay as they are)."""
    if "pairs" not in _cache:
        _cache["pairs"] = _pairs(cuda)
    pairs = list(_cache["pairs"])
    pairs.append(pairs[1])
    if bad:
        speech = dict(pairs[BAD - 1][0])
        speech["dec_target"] = speech["dec_target"].clone()
        speech["dec_target"][0, 5, 3] = float("inf")
        pairs[BAD - 1] = [speech, pairs[BAD - 1][1]]
    return pairs


def _run(cuda, mode, source, *, micro="side_by_side", nonfinite=None, stats=False, limit=None, n_updates=6, snap_after=(), end="finish"):
    """test_batch_feed_gpu._run with the guard's options.  Returns {"state", "snaps": {k: state after update k}, "skipped", "entries",
    "error": the FloatingPointError finish() raised (end="logging_outputs": that call, made INSTEAD of finish())}."""
    from speecht5_amd.criterions import SpeechT5Criterion
    from speecht5_amd.speecht5 import T5TransformerModel
    from speecht5_amd.task import SpeechT5Task
    from speecht5_amd.update import PretrainUpdate
    m, fx_s = load_golden("tiny_speech_pretrain.pt")
    _, fx_t = load_golden("tiny_text_pretrain.pt")
    args = Namespace(**m["args"])
    for k in ("dropout", "attention_dropout", "activation_dropout"):
        setattr(args, k, 0.1)
    args.encoder_layerdrop = args.decoder_layerdrop = 0.05
    Fn.set_compute_dtype(BF)
    task = SpeechT5Task(args, Task().dicts)
    model = T5TransformerModel.build_model(args, task)
    torch.nn.Module.load_state_dict(model, m["state_dict"], strict=True)
    model = model.to(cuda).train()
    crit = SpeechT5Criterion(task, loss_weights=[10, 0.1], sync_logging=False)
    Fn.manual_seed(21)
    np.random.seed(8)
    torch.manual_seed(8)
    upd = None
    out = {"snaps": {}, "entries": None, "error": None, "skipped": None}
    try:
        static = [to_dev(fx_s["sample"], cuda), to_dev(fx_t["sample"], cuda)]
        kw = {}
        if nonfinite is not None:
            kw["nonfinite"] = nonfinite
        if limit is not None:
            kw["nonfinite_limit"] = limit
        upd = PretrainUpdate(task, model, crit, static, lr=1e-3, clip_norm=1.0, graph=mode == "graph", micro=micro, device=cuda,
                             stats=stats, **kw)
        upd.set_source(list(source))
        done = 0
        if mode == "graph":
            upd.prepare_graph()
            done = 2
        else:
            Fn._S.force_static = True
        if done in snap_after:
            out["snaps"][done] = upd.state()
        while done < n_updates:
            upd.update()
            done += 1
            if done in snap_after:
                out["snaps"][done] = upd.state()
        try:
            if end == "finish":
                upd.finish()
            else:
                upd.logging_outputs(wait=True)
        except FloatingPointError as e:
            out["error"] = e
        out["state"] = upd.state()
        if nonfinite is not None:
            out["skipped"] = upd.opt.skipped()
        if stats:
            out["entries"] = upd.logging_outputs(wait=True)
        return out
    finally:
        Fn._S.force_static = False
        if upd is not None:
            upd.close()
        Fn.bf16_mirror.__init__()
        Fn.weight_cache.clear()
        Fn.set_layer_boundary_hook(None)
        Fn.set_compute_dtype(torch.float32)


_cache = {}


def _shared(cuda, key):
    """Each run once, shared by the tests, never modified."""
    if key not in _cache:
        clean, bad = (lambda: _source(cuda, False)), (lambda: _source(cuda, True))
        if key == "clean_eager_off":
            _cache[key] = _run(cuda, "eager", clean(), micro="in_turn", n_updates=5)
        elif key == "clean_eager_on":
            _cache[key] = _run(cuda, "eager", clean(), micro="in_turn", nonfinite="skip", n_updates=5)
        elif key == "clean_graph_off":
            _cache[key] = _run(cuda, "graph", clean(), n_updates=5)
        elif key == "clean_graph_on":
            _cache[key] = _run(cuda, "graph", clean(), nonfinite="skip", n_updates=5)
        elif key == "bad_eager":
            _cache[key] = _run(cuda, "eager", bad(), micro="in_turn", nonfinite="skip", stats=True, snap_after=(2, 3))
        elif key == "bad_in_turn":
            _cache[key] = _run(cuda, "graph", bad(), micro="in_turn", nonfinite="skip", snap_after=(2, 3))
        elif key == "bad_side_by_side":
            _cache[key] = _run(cuda, "graph", bad(), micro="side_by_side", nonfinite="skip", stats=True, snap_after=(2, 3))
    return _cache[key]


def _states_equal(a, b, what):
    assert a[3] == b[3], (what, a[3], b[3])
    for x, y, name in zip(a[:3], b[:3], ("parameters", "first moment", "second moment")):
        assert _same(x, y), (what, name)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_clean_source_guard_changes_nothing(cuda, mode):
    off, on = _shared(cuda, f"clean_{mode}_off"), _shared(cuda, f"clean_{mode}_on")
    assert off["state"][3] == 5 and bool(torch.isfinite(on["state"][0]).all())
    _states_equal(off["state"], on["state"], f"clean source, {mode}")
    assert on["skipped"] == 0


@pytest.mark.parametrize("arm", ["bad_eager", "bad_in_turn", "bad_side_by_side"])
def test_bad_batch_is_skipped(cuda, arm):
    r = _shared(cuda, arm)
    s2, s3 = r["snaps"][2], r["snaps"][3]
    assert (s2[3], s3[3]) == (2, 3)                      # the host counts attempts
    for x, y, name in zip(s2[:3], s3[:3], ("parameters", "first moment", "second moment")):
        assert _same(x, y), (arm, name, "changed by the skipped update")
    assert r["skipped"] == 1 and r["error"] is None
    assert r["state"][3] == 6 and not _same(r["state"][0], s3[0])       # ... and the updates behind it trained on


def test_arms_agree_after_six_updates(cuda):
    ref = _shared(cuda, "bad_eager")["state"]
    for x in ref[:3]:
        assert bool(torch.isfinite(x).all())
    for arm in ("bad_in_turn", "bad_side_by_side"):
        _states_equal(ref, _shared(cuda, arm)["state"], arm)


def test_bad_batch_without_the_guard_poisons_the_parameters(cuda):
    """What the option exists for, recorded once (and the confirmation that the planted +inf does reach the gradient)."""
    r = _run(cuda, "eager", _source(cuda, True), micro="in_turn", n_updates=3, snap_after=(2,))
    assert bool(torch.isfinite(r["snaps"][2][0]).all())
    assert not bool(torch.isfinite(r["state"][0]).all())


@pytest.mark.parametrize("arm", ["bad_eager", "bad_side_by_side"])
def test_statistics_carry_the_verdict(cuda, arm):
    entries = _shared(cuda, arm)["entries"]
    assert [e["num_updates"] for e in entries] == [1, 2, 3, 4, 5, 6]
    assert [e["skipped"] for e in entries] == [0, 0, 1, 0, 0, 0]
    assert not np.isfinite(entries[BAD - 1]["gnorm"])
    assert all(np.isfinite(e["gnorm"]) and e["gnorm"] > 0 for i, e in enumerate(entries) if i != BAD - 1)


def test_statistics_without_the_guard_have_no_such_key(cuda):
    r = _run(cuda, "eager", _source(cuda, False), micro="in_turn", stats=True, n_updates=2)
    assert len(r["entries"]) == 2 and all("skipped" not in e for e in r["entries"])
    assert sorted(r["entries"][0]) == ["clip", "gnorm", "gnorm_sq", "logging_outputs", "lr", "num_updates"]


@pytest.mark.parametrize("end", ["finish", "logging_outputs"])
def test_nonfinite_limit(cuda, end):
    r = _run(cuda, "graph", _source(cuda, True), micro="in_turn", nonfinite="skip", stats=True, limit=1, end=end)
    assert isinstance(r["error"], FloatingPointError) and f"update {BAD}" in str(r["error"]), r["error"]
    assert [e["skipped"] for e in r["entries"]] == [0, 0, 1, 0, 0, 0]       # (the entries are kept for the caller)


def test_refused_options(cuda):
    with pytest.raises(ValueError):
        _run(cuda, "eager", _source(cuda, False), nonfinite="skip", limit=1, n_updates=0)      # without stats
    with pytest.raises(ValueError):
        _run(cuda, "eager", _source(cuda, False), nonfinite="keep", n_updates=0)
