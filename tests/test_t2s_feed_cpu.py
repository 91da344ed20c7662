"""The feed and audit tables of the replayed TTS fine-tuning update (t2s), without a GPU:
1. graph.HOST_VALUES_FREE_T2S / host_values_free(), train_stats.DEVICE_LOGGED_OPTIONS["t2s"], device_logged() and
   check_feed_host_values with and without the criterion's device_ntokens option;
2. graph.BatchFeed on CPU tensors lets a t2s `ntokens` differ from batch to batch, and nothing else;
3. update.check_t2s_source's two refusals, by option name;
4. collate.TextToSpeechCollater.plan() on host ints: shapes, the live step count and its refusals, naming the item;
5. the new keywords are optional and off by default; tgt_live is refused off the t2s route before anything runs."""
import inspect
from types import SimpleNamespace

import pytest
import torch

from speecht5_amd.graph import HOST_VALUES_FREE, HOST_VALUES_FREE_T2S, BatchFeed, host_values_free


def _crit(**kw):
    return SimpleNamespace(**{"device_ntokens": True, **kw})


def _t2s(seed=0, ntokens=17, live=5, with_live=True):
    g = torch.Generator().manual_seed(seed)
    ni = {"src_tokens": torch.randint(4, 30, (2, 6), generator=g), "src_lengths": torch.tensor([6, 4]),
          "prev_output_tokens": torch.randn(2, 5, 8, generator=g), "tgt_lengths": torch.tensor([5, 3]),
          "spkembs": torch.randn(2, 4, generator=g), "task_name": "t2s"}
    if with_live:
        ni["tgt_live"] = torch.tensor([live], dtype=torch.int32)
    tgt = torch.randn(2, 10, 8, generator=g)
    return {"id": torch.LongTensor([3, 4]), "name": ["a", "b"], "net_input": ni, "labels": torch.zeros(2, 10), "dec_target": tgt,
            "dec_target_lengths": torch.tensor([10, 7]), "src_lengths": ni["src_lengths"], "task_name": "t2s", "ntokens": ntokens,
            "target": tgt}


# ---- 1 ----
def test_t2s_free_values_and_the_stats_audit():
    from speecht5_amd.train_stats import DEVICE_LOGGED_OPTIONS, LOGGED_SAMPLE_VALUES, check_feed_host_values, device_logged
    # t2s's free value lives in a table of its own (HOST_VALUES_FREE keeps the entries tests/test_ctc_pack_cpu.py pins); the feed and
    # the audit go by both
    assert HOST_VALUES_FREE_T2S == {"t2s": ("ntokens",)} and "t2s" not in HOST_VALUES_FREE
    FREE = host_values_free()
    assert FREE["t2s"] == ("ntokens",) and all(FREE[k] == v for k, v in HOST_VALUES_FREE.items()) and len(FREE) == len(HOST_VALUES_FREE) + 1
    assert DEVICE_LOGGED_OPTIONS["t2s"] == {"ntokens": "device_ntokens=True"}
    assert LOGGED_SAMPLE_VALUES["t2s"] == {"ntokens": "ntokens"}
    assert device_logged("t2s", _crit()) == ("ntokens",)
    assert device_logged("t2s", _crit(device_ntokens=False)) == ()
    assert device_logged("t2s", SimpleNamespace(speech_criterion=_crit())) == ("ntokens",)         # (SpeechT5Criterion's part)
    assert device_logged("t2s", SimpleNamespace(speech_criterion=_crit(device_ntokens=False))) == ()
    assert device_logged("s2s", _crit()) == ()                                                     # the option is t2s's alone
    check_feed_host_values(["t2s"], FREE, {"t2s": device_logged("t2s", _crit())})
    with pytest.raises(ValueError, match="t2s.*`ntokens`"):
        check_feed_host_values(["t2s"], FREE)
    with pytest.raises(ValueError, match="t2s.*`ntokens`"):
        check_feed_host_values(["t2s"], FREE, {"t2s": device_logged("t2s", _crit(device_ntokens=False))})
    with pytest.raises(ValueError, match="t2s.*sample_size"):        # no option of the t2s criterion is known for any other key
        check_feed_host_values(["t2s"], FREE, {"t2s": ("sample_size",)})
    # s2s and s2c stay refused under a source
    for name in ("s2s", "s2c"):
        assert name not in FREE and device_logged(name, _crit()) == ()


# ---- 2 ----
def test_batch_feed_lets_a_t2s_ntokens_differ_and_nothing_else():
    feed = BatchFeed([_t2s(0, ntokens=10, live=5)])
    nxt = _t2s(1, ntokens=7, live=3)
    feed.set_source([[nxt]])
    rec = feed.pull()
    assert rec.host[(0, ("ntokens",))] == 7 and feed.static[0]["ntokens"] == 7          # the static sample's log value follows the batch
    assert any(k == ("net_input", "tgt_live") for _, k in feed.paths)                   # the live count is a loaded leaf
    bad = _t2s(2)
    bad["name"] = ["a", "c"]
    feed.set_source([[bad]])
    with pytest.raises(ValueError, match=r"micro_batches\[0\]\.name"):
        feed.pull()
    feed.set_source([[_t2s(3, with_live=False)]])
    with pytest.raises(ValueError, match=r"net_input\.tgt_live.*missing"):
        feed.pull()
    # s2s has no free value: the same difference is refused
    a, b = _t2s(0, ntokens=10), _t2s(1, ntokens=7)
    for s in (a, b):
        s["task_name"] = "s2s"
    feed = BatchFeed([a])
    feed.set_source([[b]])
    with pytest.raises(ValueError, match=r"micro_batches\[0\]\.ntokens"):
        feed.pull()


# ---- 3 ----
def test_update_refuses_a_t2s_source_by_option():
    from speecht5_amd.update import check_t2s_source
    mb = [_t2s()]
    check_t2s_source(mb, _crit(), stats=True)
    check_t2s_source(mb, _crit(device_ntokens=False), stats=False)              # nothing logged from the ring: the host value is unused
    check_t2s_source([_t2s(with_live=False)], _crit(device_ntokens=False), graph=False, stats=True)      # eager: every batch as it is
    check_t2s_source([{"task_name": "s2t"}], _crit(device_ntokens=False), stats=True)
    with pytest.raises(ValueError, match="tgt_live"):
        check_t2s_source([_t2s(with_live=False)], _crit(), stats=True)
    with pytest.raises(ValueError, match="device_ntokens"):
        check_t2s_source(mb, _crit(device_ntokens=False), stats=True)
    with pytest.raises(ValueError, match=r"micro_batches\[1\].*device_ntokens"):
        check_t2s_source([{"task_name": "text_pretrain"}, _t2s()], SimpleNamespace(speech_criterion=_crit(device_ntokens=False)), stats=True)


# ---- 4 ----
def test_plan_shapes_live_count_and_refusals():
    from speecht5_amd.collate import TextToSpeechCollater as C
    assert C.plan([0, 1, 2], [11, 3, 7], [24, 13, 9], 2) == (11, 24, 12)
    assert C.plan([0, 1, 2], [11, 3, 7], [24, 13, 9], 2, (16, 32)) == (16, 32, 12)
    assert C.plan([0, 1], [4, 5], [27, 26], 2, (12, 28)) == (12, 28, 13)             # an odd longest utterance: its last frame has no step
    assert C.plan([0, 1], [4, 5], [28, 2], 2, (12, 28)) == (12, 28, 14)              # the shape filled, a one-step utterance beside it
    assert C.plan([0], [4], [7], 1, (4, 9)) == (4, 9, 7) and C.plan([0], [4], [7], 3) == (4, 7, 2)
    with pytest.raises(ValueError, match=r"item 8: 13 tokens.*12"):
        C.plan([7, 8], [12, 13], [6, 6], 2, (12, 28))
    with pytest.raises(ValueError, match=r"item 'utt-b': 29 frames.*28"):
        C.plan(["utt-a", "utt-b"], [3, 3], [28, 29], 2, (12, 28))
    with pytest.raises(ValueError, match=r"item 5: 1 frames.*reduction_factor = 2"):
        C.plan([4, 5], [3, 3], [28, 1], 2, (12, 28))
    for bad in ((12, 27), (12, 0), (0, 28), (12,), (12.0, 28), "12x28"):
        with pytest.raises(ValueError, match="fixed_shape"):
            C("cpu", fixed_shape=bad)
    assert C("cpu").fixed_shape is None and C("cpu", fixed_shape=[12, 28]).fixed_shape == (12, 28)


# ---- 5 ----
def test_new_keywords_are_optional_and_off_by_default():
    from speecht5_amd import functional as Fn
    from speecht5_amd.collate import TextToSpeechCollater
    from speecht5_amd.criterions import SpeechT5Criterion, TexttoSpeechLoss
    from speecht5_amd.modules.speech_decoder_postnet import Postnet, SpeechDecoderPostnet
    from speecht5_amd.speecht5 import T5TransformerModel
    for fn, key, default in ((TexttoSpeechLoss.__init__, "device_ntokens", False), (SpeechT5Criterion.__init__, "device_ntokens", False),
                             (Fn.postnet, "live", None), (Postnet.forward, "live", None), (SpeechDecoderPostnet.forward, "live", None),
                             (T5TransformerModel.forward, "tgt_live", None), (TextToSpeechCollater.__init__, "fixed_shape", None)):
        assert inspect.signature(fn).parameters[key].default is default, (fn, key)
    assert TexttoSpeechLoss(None, device_ntokens=True).device_ntokens is True and TexttoSpeechLoss(None).device_ntokens is False


@pytest.mark.parametrize("task_name", ["s2t", "s2s", "s2c", "speech_pretrain", "text_pretrain", None])
def test_tgt_live_is_refused_off_the_t2s_route(task_name):
    from speecht5_amd.speecht5 import T5TransformerModel
    with pytest.raises(ValueError, match="tgt_live"):        # (before `self` is touched: no model is built for this)
        T5TransformerModel.forward(None, src_tokens=torch.zeros(1, 2, dtype=torch.long), task_name=task_name,
                                   tgt_live=torch.ones(1, dtype=torch.int32))


def test_postnet_refuses_a_live_value_that_is_not_a_device_cell():
    from speecht5_amd import functional as Fn
    x = torch.zeros(1, 4, 8)
    for bad in (3, torch.tensor([3]), torch.tensor([3, 4], dtype=torch.int32)):
        with pytest.raises(ValueError, match="live"):
            Fn.postnet(x, [], True, 0.0, live=bad)
