"""ASR fine-tuning (s2t, CE + CTC) as a replayed update fed by collate.SpeechToTextCollater(fixed_shape=...), on the tiny model (bf16,
dropout 0.1, LayerDrop 0.05, span mask 0.5, channel mask 0.5; SpeechtoTextLoss(sentence_avg=True, ce_weight=0.5, ctc_weight=0.5,
report_accuracy=True, device_targets=True); one micro-batch, micro="in_turn", stats=True).  Mirrors tests/test_batch_feed_gpu.py.

Replay: six fed updates (two recorded, four replayed), every batch different, one fixed shape.  The replayed state is bit-equal to
the eager static-shape update on the same source and every logging entry `==` the eager one (ntokens, the pack kernel's count,
differs from entry to entry); numpy's and torch's CPU generators end where the eager loop leaves them.  A run with a planted fault --
every replay behind the first reuses the first replay's channel mask, what a copy baked into the graph would do -- does NOT reach
the eager state: the channel mask moves.

Freeze: freeze_encoder_updates = 4, seven updates, weight decay 0 (a frozen parameter then keeps its bits: zero gradient, zero
moments).  Without recapture the replay of update 4 raises and the state is that of three updates.  With recapture=True the seven
updates are bit-equal to seven eager ones, two graphs were captured, and the encoder's parameters are untouched through update 3 and
move afterwards."""
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from speecht5_amd import functional as Fn
from tests.util import Task, load_golden

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
S, L = 7000, 9                      # the fixed shape: samples per row, target columns (the fixture's)
# per batch: the two clips' samples and label counts (label + </s> must fit L; rows that fill it and a one-label row among them)
CLIPS = [[7000, 5200], [6100, 7000], [7000, 7000], [3900, 6600], [7000, 4800], [5600, 6900], [6400, 7000]]
LABELS = [[8, 6], [5, 8], [8, 8], [3, 7], [1, 8], [6, 2], [7, 4]]


def _batches(cuda, n):
    """n batches of synthetic clips through the new collater, one fixed shape; the first one a second time as the update's static
    sample (the constructor's tensors are overwritten by every load)."""
    from speecht5_amd.collate import SpeechToTextCollater
    g = torch.Generator().manual_seed(4321)
    coll = SpeechToTextCollater(cuda, fixed_shape=(S, L))
    items = []
    for k in range(n):
        items.append([{"id": 2 * k + i, "source": torch.randn(CLIPS[k][i], generator=g).to(cuda),
                       "label_list": [torch.randint(4, 34, (LABELS[k][i],), generator=g).to(cuda)]} for i in range(2)])
    out = [[coll(it)] for it in items]
    static = [coll(items[0])]
    torch.cuda.synchronize()
    for k, (b,) in enumerate(out):
        assert tuple(b["net_input"]["source"].shape) == (2, S) and tuple(b["target"].shape) == (2, L) and b["ntokens"] == sum(LABELS[k])
        assert torch.equal(b["net_input"]["padding_mask"]._st5_host, torch.arange(S)[None, :] >= torch.tensor(CLIPS[k])[:, None])
        assert torch.equal(b["net_input"]["padding_mask"].cpu(), b["net_input"]["padding_mask"]._st5_host)
    return out, static


def _rng_state():
    st = np.random.get_state()
    return st[1].copy(), st[2], torch.get_rng_state().clone()


def _run(cuda, mode, *, n_updates=6, freeze=0, recapture=False, prefetch=False, plant=False, weight_decay=0.01, expect_raise=None):
    """-> dict(state, entries, rng, pulls, captures, snaps {update count: encoder parameters}, raised)."""
    from speecht5_amd.criterions import SpeechtoTextLoss
    from speecht5_amd.speecht5 import T5TransformerModel
    from speecht5_amd.task import SpeechT5Task
    from speecht5_amd.update import PretrainUpdate
    m, _ = load_golden("tiny_s2t.pt")
    args = Namespace(**m["args"])
    for k in ("dropout", "attention_dropout", "activation_dropout"):
        setattr(args, k, 0.1)
    args.encoder_layerdrop = args.decoder_layerdrop = 0.05
    args.mask_prob, args.mask_channel_prob = 0.5, 0.5
    args.freeze_encoder_updates = freeze
    Fn.set_compute_dtype(BF)
    task = SpeechT5Task(args, Task().dicts)
    model = T5TransformerModel.build_model(args, task)
    torch.nn.Module.load_state_dict(model, m["state_dict"], strict=True)
    model = model.to(cuda).train()
    assert model.speech_encoder_prenet.mask_channel_prob == 0.5 and model.encoder.freeze_encoder_updates == freeze
    crit = SpeechtoTextLoss(SimpleNamespace(zero_infinity=True), task, sentence_avg=True, label_smoothing=0.1, report_accuracy=True,
                            ce_weight=0.5, ctc_weight=0.5, sync_logging=False, device_targets=True)
    source, static = _batches(cuda, n_updates)
    frozen = [p for mod in (model.encoder.layers, model.speech_encoder_prenet) for p in mod.parameters()]
    Fn.manual_seed(21)
    np.random.seed(8)
    torch.manual_seed(8)
    upd, real_stage = None, Fn.stage_host
    out = {"snaps": {}, "raised": None}

    def snap():
        torch.cuda.synchronize()
        out["snaps"][upd.opt.t] = [p.detach().clone() for p in frozen]

    def planted_stage(producer, device):
        # every replay behind the first reuses the first replay's channel mask; the producer still runs (numpy's stream advances as
        # before).  A producer object's calls: the recording step that made it, then once per prepared replay.
        if getattr(producer, "__name__", "") != "draw_channels":
            return real_stage(producer, device)
        box = {"calls": 0}

        def stale():
            mask = producer()
            box["calls"] += 1
            if box["calls"] == 2:
                box["kept"] = mask
            return box["kept"] if box["calls"] > 2 else mask
        return real_stage(stale, device)
    try:
        upd = PretrainUpdate(task, model, crit, static, lr=1e-3, clip_norm=1.0, weight_decay=weight_decay, graph=mode == "graph",
                             micro="in_turn", prefetch_host=prefetch, device=cuda, stats=True, recapture=recapture)
        pulled = []

        def src():
            for b in source:
                pulled.append(b)
                yield b
        upd.set_source(src())
        snap()
        if plant:
            Fn.stage_host = planted_stage
        if mode == "graph":
            upd.prepare_graph()
            snap()
            while upd.opt.t < n_updates:
                if expect_raise is not None and upd.opt.t == expect_raise - 1:
                    with pytest.raises(RuntimeError) as e:
                        upd.update()
                    out["raised"] = str(e.value)
                    with pytest.raises(RuntimeError):      # (and again: nothing was enqueued, pulled or counted by the refusal)
                        upd.update()
                    break
                upd.update()
                snap()
            upd.finish()
        else:
            Fn._S.force_static = True
            for _ in range(n_updates):
                upd.eager_update()
                snap()
        out["rng"] = _rng_state()
        out["entries"] = upd.logging_outputs(wait=True)
        out["state"] = upd.state()
        out["pulls"], out["captures"], out["host_ntokens"] = len(pulled), upd.captures, [b[0]["ntokens"] for b in source]
        return out
    finally:
        Fn.stage_host = real_stage
        Fn._S.force_static = False
        if upd is not None:
            upd.close()
        Fn.bf16_mirror.__init__()
        Fn.weight_cache.clear()
        Fn.set_layer_boundary_hook(None)
        Fn.set_compute_dtype(torch.float32)


_cache = {}


def _shared(cuda, key):
    """Each reference run once, shared by the tests, never modified."""
    if key not in _cache:
        if key == "eager":
            _cache[key] = _run(cuda, "eager")
        elif key == "replay":
            _cache[key] = _run(cuda, "graph")
        elif key == "eager_freeze":
            _cache[key] = _run(cuda, "eager", n_updates=7, freeze=4, weight_decay=0.0)
    return _cache[key]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _state_equal(ref, got):
    return ref[3] == got[3] and all(_same(x, y) for x, y in zip(ref[:3], got[:3]))


def _assert_state_equal(ref, got, n, what):
    assert ref[3] == got[3] == n and torch.isfinite(got[0]).all(), (what, ref[3], got[3])
    for x, y, name in zip(ref[:3], got[:3], ("parameters", "first moment", "second moment")):
        assert _same(x, y), (what, name, float((x - y).abs().max()))


# ---- replay ----
def test_replayed_s2t_update_equals_eager(cuda):
    ref, got = _shared(cuda, "eager"), _shared(cuda, "replay")
    assert ref["pulls"] == got["pulls"] == 6 and got["captures"] == 1
    _assert_state_equal(ref["state"], got["state"], 6, "s2t, fed, in turn")


def test_replayed_s2t_update_with_the_helper_thread(cuda):
    ref = _shared(cuda, "eager")
    got = _run(cuda, "graph", prefetch=True)
    _assert_state_equal(ref["state"], got["state"], 6, "s2t, fed, in turn, prefetch")
    assert got["entries"] == ref["entries"]


def test_every_logging_entry_equals_the_eager_one(cuda):
    ref, got = _shared(cuda, "eager"), _shared(cuda, "replay")
    assert len(ref["entries"]) == len(got["entries"]) == 6
    for k, (a, b) in enumerate(zip(ref["entries"], got["entries"])):
        assert a == b, (k, a, b)
    nt = [e["logging_outputs"][0]["s2t"]["ntokens"] for e in got["entries"]]
    assert nt == got["host_ntokens"] == [sum(v) for v in LABELS[:6]] and len(set(nt)) > 3      # per batch, from the device
    assert [e["logging_outputs"][0]["ntokens"] for e in got["entries"]] == nt
    for e in got["entries"]:
        log = e["logging_outputs"][0]["s2t"]
        assert log["sample_size"] == 2 and log["nsentences"] == 2 and log["ctc_loss"] > 0 and log["ce_loss"] > 0 and log["total"] > 0


def test_host_random_streams_end_where_the_eager_loop_leaves_them(cuda):
    ref, got = _shared(cuda, "eager")["rng"], _shared(cuda, "replay")["rng"]
    assert np.array_equal(ref[0], got[0]) and ref[1] == got[1], "numpy's generator"
    assert torch.equal(ref[2], got[2]), "torch's CPU generator"


def test_the_channel_mask_moves_with_every_replay(cuda):
    """The planted fault: replays 2.. reuse replay 1's channel mask.  Its first three updates (two recorded, the first replay) are
    the eager ones; from the fourth on the state leaves the eager trajectory -- which the unplanted replay stays on."""
    ref, good = _shared(cuda, "eager"), _shared(cuda, "replay")
    bad = _run(cuda, "graph", plant=True)
    assert bad["state"][3] == 6 and torch.isfinite(bad["state"][0]).all()
    assert _state_equal(ref["state"], good["state"]) and not _state_equal(ref["state"], bad["state"])
    assert bad["entries"][:3] == ref["entries"][:3] and bad["entries"][3:] != ref["entries"][3:]
    r, b = ref["rng"], bad["rng"]
    assert np.array_equal(r[0], b[0]) and r[1] == b[1]      # (the plant draws as often as the real producer)


# ---- freeze ----
def test_a_replay_across_the_freeze_boundary_is_refused(cuda):
    ref = _shared(cuda, "eager_freeze")
    got = _run(cuda, "graph", n_updates=7, freeze=4, weight_decay=0.0, expect_raise=4)
    msg = got["raised"]
    assert "freeze_encoder_updates" in msg and "update 3" in msg and "update 4" in msg, msg
    assert got["state"][3] == 3 and got["pulls"] == 3 and got["captures"] == 1
    assert [e["num_updates"] for e in got["entries"]] == [1, 2, 3] and got["entries"] == ref["entries"][:3]
    for a, b in zip(ref["snaps"][3], got["snaps"][3]):
        assert _same(a, b)


def test_recapture_at_the_freeze_boundary_equals_eager(cuda):
    ref = _shared(cuda, "eager_freeze")
    got = _run(cuda, "graph", n_updates=7, freeze=4, weight_decay=0.0, recapture=True)
    assert got["captures"] == 2 and got["pulls"] == ref["pulls"] == 7
    _assert_state_equal(ref["state"], got["state"], 7, "freeze 4, recapture")
    assert got["entries"] == ref["entries"] and [e["num_updates"] for e in got["entries"]] == list(range(1, 8))
    assert sorted(got["snaps"]) == [0, 2, 3, 5, 6, 7]       # (the update() that met the boundary ran updates 4 and 5 as recording steps)
    for run in (ref, got):
        for t, params in run["snaps"].items():
            moved = [not _same(a, b) for a, b in zip(run["snaps"][0], params)]
            assert (not any(moved)) if t <= 3 else (sum(moved) > len(moved) // 2), (t, sum(moved), len(moved))
    for t in got["snaps"]:
        assert all(_same(a, b) for a, b in zip(ref["snaps"][t], got["snaps"][t])), t
    r, g = ref["rng"], got["rng"]
    assert np.array_equal(r[0], g[0]) and r[1] == g[1] and torch.equal(r[2], g[2])


def test_recapture_needs_the_host_side_in_step(cuda):
    from speecht5_amd.update import PretrainUpdate
    with pytest.raises(ValueError, match="prefetch_host"):
        PretrainUpdate(None, torch.nn.Linear(2, 2), None, [], recapture=True)
