"""Save and resume on the GPU (update.PretrainUpdate.state_dict / load_state_dict / snapshot / save_checkpoint, checkpoint.py): the
update of tests/test_batch_feed_gpu.py (tiny model, bf16, dropout 0.1, LayerDrop 0.05) with nonfinite="skip", eight fed updates, one
+inf planted in the mel target of batches 2 and 5 (counted from 0: updates 3 and 6 are skipped, one on each side of the save).

A run that is stopped after update 4, whose every restorable piece of state is then scrambled, and that is continued from the
checkpoint in NEW objects ends bit-equal to the run that was never stopped: parameters, both moments, the step count, every model
buffer, the guard block's skip count, the dropout seed counter, numpy's and torch's host generators, torch's device generator and the
bf16 image -- eagerly through a file, into a replayed graph from state_dict(), and from a snapshot() taken while four more updates
were enqueued behind it."""
import copy
from argparse import Namespace

import numpy as np
import pytest
import torch

from speecht5_amd import checkpoint
from speecht5_amd import functional as Fn
from tests.test_batch_feed_gpu import _pairs, _same
from tests.util import Task, load_golden, to_dev

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N = 8
BAD = (2, 5)      # batches (0-based) with one +inf in the speech micro-batch's mel target
_cache = {}


def _source(cuda):
    """Eight pairs: the five of tests/test_batch_feed_gpu.py, cycled (its SRC_LEN / DEC_LEN describe five); the bad ones are copies."""
    if "source" not in _cache:
        five = _pairs(cuda)
        pairs = [five[k % len(five)] for k in range(N)]
        for k in BAD:
            speech = dict(pairs[k][0])
            speech["dec_target"] = speech["dec_target"].clone()
            speech["dec_target"][0, 5, 3] = float("inf")
            pairs[k] = [speech, pairs[k][1]]
        _cache["source"] = pairs
    return _cache["source"]


def _end_state(upd):
    upd.finish()
    state = upd.state()
    return {"state": state, "buffers": {k: v.detach().clone() for k, v in upd.model.named_buffers()}, "skipped": upd.opt.skipped(),
            "counter": (Fn._S.seed, Fn._S.counter), "numpy": np.random.get_state(), "torch_cpu": torch.get_rng_state().clone(),
            "torch_device": torch.cuda.get_rng_state(upd.device).clone(), "wflat": upd.opt.wflat.clone(), "n": upd.n,
            "pulled": upd.batches_pulled}


def _run(cuda, *, mode, micro="side_by_side", prefetch=False, resume=None, first=0, last=N, after=None, end=None, build_only=False):
    """Updates first + 1 .. last of the fed run, eagerly or as a graph (two recording steps, then replays).  resume: a state
    dictionary -- everything a load must restore is scrambled first, then it is loaded into the new update.  after(upd, k) runs behind
    update k; end(upd) in front of close() and its return value is returned in place of the end state."""
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
    if resume is None:
        Fn.manual_seed(21)
        np.random.seed(8)
        torch.manual_seed(8)
    else:
        Fn.manual_seed(999)
        np.random.seed(0)
        torch.manual_seed(0)
        with torch.no_grad():
            for t in list(model.parameters()) + list(model.buffers()):
                t.add_(1)
    upd = None
    try:
        static = [to_dev(fx_s["sample"], cuda), to_dev(fx_t["sample"], cuda)]
        upd = PretrainUpdate(task, model, crit, static, lr=1e-3, clip_norm=1.0, graph=mode == "graph", micro=micro, prefetch_host=prefetch,
                             device=cuda, nonfinite="skip")
        if build_only:
            return build_only(upd)
        if resume is not None:
            upd.load_state_dict(resume)
            assert upd.n == first and upd.opt.t == first and upd.batches_pulled == first
        upd.set_source(_source(cuda)[first:])
        done = first
        if mode == "graph":
            upd.prepare_graph()
            done += 2
        else:
            Fn._S.force_static = True
        while done < last:
            upd.update()
            done += 1
            if after is not None:
                after(upd, done)
        return end(upd) if end is not None else _end_state(upd)
    finally:
        Fn._S.force_static = False
        if upd is not None:
            upd.close()
        Fn.bf16_mirror.__init__()
        Fn.weight_cache.clear()
        Fn.set_layer_boundary_hook(None)
        Fn.set_compute_dtype(torch.float32)


def _shared(cuda, key):
    """Each uninterrupted run once, shared by the tests, never modified."""
    if key not in _cache:
        if key == "eager":
            _cache[key] = _run(cuda, mode="eager", micro="in_turn")
        else:
            _cache[key] = _run(cuda, mode="graph", micro=key)
    return _cache[key]


def _assert_same_end(ref, got, what):
    assert ref["state"][3] == got["state"][3] == N and ref["n"] == got["n"] == N, (what, ref["state"][3], got["state"][3])
    assert bool(torch.isfinite(got["state"][0]).all())
    for x, y, name in zip(ref["state"][:3], got["state"][:3], ("parameters", "first moment", "second moment")):
        assert _same(x, y), (what, name)
    assert sorted(ref["buffers"]) == sorted(got["buffers"]) and len(ref["buffers"]) > 0
    for k in ref["buffers"]:
        assert _same(ref["buffers"][k].reshape(-1), got["buffers"][k].reshape(-1)), (what, "buffer", k)      # (reshape: 0-dim counters)
    assert ref["skipped"] == got["skipped"] == len(BAD), (what, ref["skipped"], got["skipped"])
    assert ref["counter"] == got["counter"], (what, ref["counter"], got["counter"])
    a, b = ref["numpy"], got["numpy"]
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:], (what, "numpy's generator")
    assert torch.equal(ref["torch_cpu"], got["torch_cpu"]), (what, "torch's CPU generator")
    assert torch.equal(ref["torch_device"], got["torch_device"]), (what, "torch's device generator")
    assert _same(ref["wflat"], got["wflat"]), (what, "bf16 image")
    assert got["pulled"] == N


def _saved_file(cuda, tmp_path_factory):
    """Arm B of the eager test: four updates, save_checkpoint, close.  The file is shared with the refusal tests."""
    if "file" not in _cache:
        path = tmp_path_factory.mktemp("ckpt") / "c.pt"

        def end(upd):
            upd.save_checkpoint(path)
            return upd.opt.skipped()
        assert _run(cuda, mode="eager", micro="in_turn", last=4, end=end) == 1
        _cache["file"] = path
    return _cache["file"]


def test_resume_eager_through_a_file(cuda, tmp_path_factory):
    ref = _shared(cuda, "eager")
    path = _saved_file(cuda, tmp_path_factory)
    assert set(torch.load(path, weights_only=True)) == {"model", "optimizer", "extra_state", "digest"}
    sd = checkpoint.load_checkpoint(path)
    m, _ = load_golden("tiny_speech_pretrain.pt")
    assert set(sd["model"]) == set(m["state_dict"])          # the reference's key set: the model entry loads as any checkpoint does
    assert sd["extra_state"]["num_updates"] == 4 and sd["extra_state"]["batches_pulled"] == 4 and sd["optimizer"]["t"] == 4
    assert sd["optimizer"]["guard"][3] == 4 and "torch_device" in sd["extra_state"]
    got = _run(cuda, mode="eager", micro="in_turn", resume=sd, first=4)
    _assert_same_end(ref, got, "eager, resumed from a file")


@pytest.mark.parametrize("micro", ["side_by_side", "in_turn"])
def test_resume_into_a_replay(cuda, micro):
    ref = _shared(cuda, micro)
    sd = _run(cuda, mode="graph", micro=micro, last=4, end=lambda upd: upd.state_dict())
    got = _run(cuda, mode="graph", micro=micro, resume=sd, first=4)
    _assert_same_end(ref, got, f"{micro}, resumed into a replay")


def test_snapshot_under_way(cuda):
    micro = "side_by_side"
    ref = _shared(cuda, micro)
    seen = {}

    def after(upd, k):
        if k == 4:
            seen["ref"] = upd.state()
            seen["buffers"] = {n: b.detach().clone() for n, b in upd.model.named_buffers()}
            seen["handle"] = upd.snapshot()
            with pytest.raises(RuntimeError, match="in flight"):
                upd.snapshot()
            seen["handle"].done()                  # (never waits; either answer is legal here)

    def end(upd):
        sd = seen["handle"].result()               # updates 5 to 8 were enqueued with no wait in between
        assert seen["handle"].done()
        return sd, _end_state(upd)
    sd, got = _run(cuda, mode="graph", micro=micro, after=after, end=end)
    _assert_same_end(ref, got, "the run that took a snapshot")                       # the snapshot changed nothing
    segs = checkpoint.segments_of(checkpoint.verify(sd))
    for x, name in zip(seen["ref"][:3], ("pflat", "m", "v")):
        assert _same(x.cpu(), segs[name]), (name, "a later update leaked into the snapshot")
    assert sd["optimizer"]["t"] == seen["ref"][3] == 4 and sd["extra_state"]["num_updates"] == 4
    for n, b in seen["buffers"].items():
        assert _same(b.cpu().reshape(-1), sd["model"][n].reshape(-1)) and b.shape == sd["model"][n].shape, ("buffer", n)
    assert not _same(seen["ref"][0], ref["state"][0])
    cont = _run(cuda, mode="graph", micro=micro, resume=sd, first=4)
    _assert_same_end(ref, cont, "resumed from the snapshot")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refused_save_points(cuda):
    def staged(upd):
        upd.set_source(_source(cuda))
        upd.prepare_graph()
        for fn in (upd.state_dict, upd.snapshot, lambda: upd.save_checkpoint("/nonexistent/c.pt")):
            with pytest.raises(RuntimeError, match="first replay after the capture is already staged"):
                fn()
        with pytest.raises(RuntimeError, match=r"load before prepare_graph\(\)"):
            upd.load_state_dict({})
        upd.update()
        assert upd.state_dict()["extra_state"]["num_updates"] == 3
    _run(cuda, mode="graph", build_only=staged)

    def ahead(upd):
        upd.set_source(_source(cuda))
        upd.prepare_graph()
        upd.update()
        for fn in (upd.state_dict, upd.snapshot):
            with pytest.raises(RuntimeError, match="prefetch_host"):
                fn()
    _run(cuda, mode="graph", prefetch=True, build_only=ahead)


def test_refused_loads(cuda, tmp_path_factory):
    sd = checkpoint.load_checkpoint(_saved_file(cuda, tmp_path_factory))

    def loads(upd):
        before = upd.state()
        name, off, n = sd["optimizer"]["layout"][3]
        bad = copy.deepcopy(sd)
        bad["optimizer"]["layout"][3][0] = name + "_renamed"
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            upd.load_state_dict(bad)
        bad = copy.deepcopy(sd)
        bad["optimizer"]["layout"][3][2] = n - 1
        with pytest.raises(ValueError, match=name.replace(".", r"\.") + " has"):
            upd.load_state_dict(bad)
        bad = copy.deepcopy(sd)
        bad["optimizer"]["betas"] = [0.9, 0.999]
        with pytest.raises(ValueError, match="betas"):
            upd.load_state_dict(bad)
        for x, y in zip(before[:3], upd.state()[:3]):
            assert _same(x, y)                      # a refused load changed nothing
        bad = copy.deepcopy(sd)
        bad["digest"]["wflat"] ^= 1
        with pytest.raises(ValueError, match="rebuilt bf16 image differs"):
            upd.load_state_dict(bad)
    _run(cuda, mode="eager", build_only=loads)


# ---- off means off -----------------------------------------------------------------------------------------------------------------
def test_nothing_is_launched_or_allocated_without_the_new_methods(cuda):
    from speecht5_amd import hip
    calls, real = [], hip.lib

    class Recording:
        def __getattr__(self, name):
            fn = getattr(real(), name)
            if name.startswith("st5_"):
                calls.append(name)
            return fn

    def run(upd):
        upd.set_source(_source(cuda))
        Fn._S.force_static = True
        hip.lib = lambda: Recording()
        try:
            upd.update()
            upd.update()
            two = list(calls)
            del calls[:]
            assert upd._shadow is None and upd._snapshot is None
            h = upd.snapshot()
            snap = list(calls)
            del calls[:]
            upd.update()
            third = list(calls)
        finally:
            hip.lib = real
        h.result()
        # an eager fed update trains on the batch's own tensors: no load kernel at all, and never a digest
        assert len(two) > 100 and "st5_state_digest" not in two and "st5_batch_load" not in two
        assert snap == ["st5_batch_load", "st5_state_digest"]
        assert "st5_state_digest" not in third and "st5_batch_load" not in third and len(third) > 50
    _run(cuda, mode="eager", micro="in_turn", build_only=run)
