"""TTS fine-tuning (t2s, L1 + BCE + guided attention) as a replayed update fed by collate.TextToSpeechCollater(fixed_shape=...), on the
tiny model (bf16, every dropout 0.1 -- the post-net's included; TexttoSpeechLoss(use_guided_attn_loss=True, device_ntokens=True); one
micro-batch, micro="in_turn", stats=True).  Mirrors tests/test_s2t_replay_gpu.py.

Six fed updates (two recorded, four replayed) over six batches whose longest utterances are 24, 28, 13, 6, 27 and 21 frames in one
fixed shape (12, 28): the live frame count of the mel post-net -- a device cell the batch load refreshes -- differs from replay to
replay.  Parameters, both Adam moments and the BatchNorm buffers are byte-equal to eager_update() on the same source; every logging
entry `==` the eager one, `ntokens` differing from entry to entry and equal to the collater's host count; numpy's and torch's CPU
generators end where the eager loop leaves them; the same with the helper thread.  update.check_t2s_source's two refusals."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from speecht5_amd import functional as Fn
from tests.util import Task, load_golden

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
VOCAB = 30
N, L, R = 12, 28, 2                 # the fixed shape: text columns, mel frames; the fixture's reduction factor
FRAMES = [[24, 11, 17], [28, 9, 15], [13, 12, 7], [6, 5, 4], [27, 26, 2], [21, 20, 3], [24, 24, 24]]
TOKENS = [[12, 5, 7], [1, 9, 4], [3, 3, 3], [12, 1, 6], [8, 2, 11], [5, 5, 10], [4, 4, 4]]


def _items(cuda, k, spk_dim, g):
    # (no audio_name: the batch's `name` list is a host value the feed compares, graph.HOST_VALUES_FREE_T2S frees `ntokens` alone)
    return [{"id": 3 * k + i,
             "source": [torch.cat([torch.randint(4, 4 + VOCAB, (n - 1,), generator=g), torch.tensor([2])]).to(cuda)],
             "target": (torch.randn(f, 80, generator=g) * 0.5 - 1).to(cuda), "spkembs": torch.randn(spk_dim, generator=g).to(cuda)}
            for i, (f, n) in enumerate(zip(FRAMES[k], TOKENS[k]))]


def _batches(cuda, n, spk_dim, fixed=True):
    """n batches of synthetic utterances through the collater, one fixed shape; the first one a second time as the update's static
    sample (the constructor's tensors are overwritten by every load)."""
    from speecht5_amd.collate import TextToSpeechCollater
    g = torch.Generator().manual_seed(2468)
    coll = TextToSpeechCollater(cuda, pad_idx=1, reduction_factor=R, fixed_shape=(N, L) if fixed else None)
    items = [_items(cuda, k, spk_dim, g) for k in range(n)]
    out = [[coll(it)] for it in items]
    static = [coll(items[0])]
    torch.cuda.synchronize()
    if fixed:
        for k, (b,) in enumerate(out):
            assert tuple(b["dec_target"].shape) == (3, L, 80) and tuple(b["net_input"]["src_tokens"].shape) == (3, N)
            assert b["ntokens"] == sum(TOKENS[k]) and int(b["net_input"]["tgt_live"]) == max(FRAMES[k]) // R
    return out, static


def _rng_state():
    st = np.random.get_state()
    return st[1].copy(), st[2], torch.get_rng_state().clone()


def _build(cuda):
    from speecht5_amd.speecht5 import T5TransformerModel
    from speecht5_amd.task import SpeechT5Task
    m, _ = load_golden("tiny_t2s.pt")
    args = Namespace(**m["args"])
    for k in ("dropout", "attention_dropout", "activation_dropout", "dprenet_dropout_rate", "postnet_dropout_rate",
              "transformer_enc_positional_dropout_rate", "transformer_dec_positional_dropout_rate", "eprenet_dropout_rate"):
        setattr(args, k, 0.1)
    Fn.set_compute_dtype(BF)
    task = SpeechT5Task(args, Task().dicts)
    model = T5TransformerModel.build_model(args, task)
    torch.nn.Module.load_state_dict(model, m["state_dict"], strict=True)
    model = model.to(cuda).train()
    model.use_codebook = False
    assert model.speech_decoder_postnet.postnet.dropout_rate == 0.1 and args.reduction_factor == R
    return args, task, model


def _crit(task, device_ntokens=True):
    from speecht5_amd.criterions import TexttoSpeechLoss
    return TexttoSpeechLoss(task, False, use_guided_attn_loss=True, guided_attn_loss_sigma=0.4, guided_attn_loss_lambda=10.0,
                            sync_logging=False, device_ntokens=device_ntokens)


def _cleanup(upd):
    Fn._S.force_static = False
    if upd is not None:
        upd.close()
    Fn.bf16_mirror.__init__()
    Fn.weight_cache.clear()
    Fn.set_layer_boundary_hook(None)
    Fn.set_compute_dtype(torch.float32)


def _run(cuda, mode, *, n_updates=6, prefetch=False):
    """-> dict(state, buffers, entries, rng, pulls, captures, host_ntokens)."""
    from speecht5_amd.update import PretrainUpdate
    upd = None
    try:
        args, task, model = _build(cuda)
        source, static = _batches(cuda, n_updates, args.spk_embed_dim)
        Fn.manual_seed(21)
        np.random.seed(8)
        torch.manual_seed(8)
        upd = PretrainUpdate(task, model, _crit(task), static, lr=1e-3, clip_norm=1.0, graph=mode == "graph", micro="in_turn",
                             prefetch_host=prefetch, device=cuda, stats=True)
        pulled = []

        def src():
            for b in source:
                pulled.append(b)
                yield b
        upd.set_source(src())
        if mode == "graph":
            upd.prepare_graph()
            while upd.opt.t < n_updates:
                upd.update()
            upd.finish()
        else:
            Fn._S.force_static = True
            for _ in range(n_updates):
                upd.eager_update()
        torch.cuda.synchronize()
        out = {"rng": _rng_state(), "entries": upd.logging_outputs(wait=True), "state": upd.state(), "pulls": len(pulled),
               "captures": upd.captures, "host_ntokens": [b[0]["ntokens"] for b in source],
               "buffers": {n: b.detach().clone() for n, b in model.named_buffers() if "running_" in n or "num_batches_tracked" in n}}
        return out
    finally:
        _cleanup(upd)


_cache = {}


def _shared(cuda, key):
    """Each reference run once, shared by the tests, never modified."""
    if key not in _cache:
        _cache[key] = _run(cuda, "eager" if key == "eager" else "graph")
    return _cache[key]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _assert_state_equal(ref, got, n, what):
    assert ref["state"][3] == got["state"][3] == n and torch.isfinite(got["state"][0]).all(), (what, ref["state"][3], got["state"][3])
    for x, y, name in zip(ref["state"][:3], got["state"][:3], ("parameters", "first moment", "second moment")):
        assert _same(x, y), (what, name, float((x - y).abs().max()))
    assert set(ref["buffers"]) == set(got["buffers"]) and len(ref["buffers"]) >= 15
    for name in ref["buffers"]:
        assert _same(ref["buffers"][name], got["buffers"][name]), (what, name)


def test_replayed_t2s_update_equals_eager(cuda):
    ref, got = _shared(cuda, "eager"), _shared(cuda, "replay")
    assert ref["pulls"] == got["pulls"] == 6 and got["captures"] == 1
    _assert_state_equal(ref, got, 6, "t2s, fed, in turn")
    m, _ = load_golden(None)
    post = [n for n in got["buffers"] if "speech_decoder_postnet" in n]
    assert len(post) == 15
    for n in post:      # the post-net's BatchNorm buffers saw six batches
        if "num_batches_tracked" in n:
            assert int(got["buffers"][n]) == int(m["state_dict"][n]) + 6
        else:
            assert not torch.equal(got["buffers"][n].cpu(), m["state_dict"][n]), n


def test_replayed_t2s_update_with_the_helper_thread(cuda):
    ref = _shared(cuda, "eager")
    got = _run(cuda, "graph", prefetch=True)
    _assert_state_equal(ref, got, 6, "t2s, fed, in turn, prefetch")
    assert got["entries"] == ref["entries"]


def test_every_logging_entry_equals_the_eager_one(cuda):
    ref, got = _shared(cuda, "eager"), _shared(cuda, "replay")
    assert len(ref["entries"]) == len(got["entries"]) == 6
    for k, (a, b) in enumerate(zip(ref["entries"], got["entries"])):
        assert a == b, (k, a, b)
    nt = [e["logging_outputs"][0]["t2s"]["ntokens"] for e in got["entries"]]
    assert nt == got["host_ntokens"] == [sum(v) for v in TOKENS[:6]] and len(set(nt)) > 3      # per batch, from the device
    assert [e["logging_outputs"][0]["ntokens"] for e in got["entries"]] == nt
    for e in got["entries"]:
        log = e["logging_outputs"][0]["t2s"]
        assert log["sample_size"] == 1 and log["nsentences"] == 3
        assert log["l1_loss"] > 0 and log["bce_loss"] > 0 and log["enc_dec_attn_loss"] > 0 and log["loss"] > log["l1_loss"]


def test_host_random_streams_end_where_the_eager_loop_leaves_them(cuda):
    ref, got = _shared(cuda, "eager")["rng"], _shared(cuda, "replay")["rng"]
    assert np.array_equal(ref[0], got[0]) and ref[1] == got[1], "numpy's generator"
    assert torch.equal(ref[2], got[2]), "torch's CPU generator"


def test_a_t2s_source_is_refused_by_option(cuda):
    from speecht5_amd.update import PretrainUpdate
    made = []

    def make(fixed, device_ntokens, graph, stats):
        args, task, model = _build(cuda)
        source, static = _batches(cuda, 1, args.spk_embed_dim, fixed=fixed)
        made.append(PretrainUpdate(task, model, _crit(task, device_ntokens), static, graph=graph, micro="in_turn", prefetch_host=False,
                                   device=cuda, stats=stats))
        return made[-1], source
    try:
        # an own-length batch carries no live count: nothing tells the post-net which frames the padding added
        upd, source = make(False, True, True, True)
        with pytest.raises(ValueError, match="tgt_live"):
            upd.set_source(iter(source))
        # the criterion's default logs the sample's host ntokens
        upd, source = make(True, False, True, True)
        with pytest.raises(ValueError, match="device_ntokens"):
            upd.set_source(iter(source))
        # ... which nothing reads without the statistics ring; and an eager update runs every batch as it is
        upd, source = make(True, False, True, False)
        upd.set_source(iter(source))
        upd, source = make(False, False, False, True)
        upd.set_source(iter(source))
    finally:
        for upd in made:
            upd.close()
        _cleanup(None)
