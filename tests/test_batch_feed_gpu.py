"""update.PretrainUpdate.set_source on the GPU (tiny model, bf16, dropout 0.1, LayerDrop 0.05): five distinct batch pairs fed to the
replayed update -- in turn and side by side, with and without the host prefetch thread -- leave parameters, both Adam moments and the
step count bit-equal to the eager static-shape update pulling the same source under the same seeds.  The eager arm runs each batch
directly on the batch's own tensors (no load kernel, no static input, no mirror re-pointing): it is independent of everything the
feed adds.  Also: feeding the recorded pair itself equals the replay without a source bit for bit; the data really reaches the step;
the span mask of a replayed update respects THAT update's padding (the stale-mirror case)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from speecht5_amd import functional as Fn
from tests.util import Task, load_golden, to_dev

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
# speech rows' valid samples and log-mel frames per pair: pairs 1, 3 and 4 are right-padded, each differently; pairs 2, 3, 4 are the
# replayed ones (the two recording steps take pairs 0 and 1)
SRC_LEN = [[6000, 6000], [6000, 4200], [6000, 6000], [2400, 6000], [6000, 3000]]
DEC_LEN = [[24, 24], [24, 16], [24, 24], [10, 24], [24, 12]]
R = 2    # the tiny model's reduction factor (prev_output_tokens has 12 of dec_target's 24 frames)


def _pairs(cuda, n=5):
    """Five (speech, text) pairs in the fixtures' shapes: waveforms and speaker embeddings re-drawn, unit labels and text tokens
    re-drawn inside their dictionaries, rows permuted; padded speech rows as the collater builds them (zeros behind the length,
    padding_mask, tgt_lengths = dec_target_lengths // r, stop labels 1.0 from the last frame on, decoder input = frames r-1, 2r-1,
    ... shifted right behind a zero frame)."""
    _, fx_s = load_golden("tiny_speech_pretrain.pt")
    _, fx_t = load_golden("tiny_text_pretrain.pt")
    g = torch.Generator().manual_seed(1234)
    dicts = Task().dicts
    n_units, n_text = len(dicts["hubert"][0]), len(dicts["text"]) - 2
    out = []
    for k in range(n):
        s, t = fx_s["sample"], fx_t["sample"]
        B, S = s["net_input"]["source"].shape
        perm = torch.randperm(B, generator=g)
        src_len, dec_len = torch.tensor(SRC_LEN[k]), torch.tensor(DEC_LEN[k])
        pm = torch.arange(S)[None, :] >= src_len[:, None]
        L = s["dec_target"].shape[1]
        fr = torch.arange(L)[None, :]
        dec = s["dec_target"].index_select(0, perm) * (fr < dec_len[:, None]).unsqueeze(-1)
        prev = torch.zeros_like(s["net_input"]["prev_output_tokens"])
        prev[:, 1:] = dec[:, R - 1::R][:, :prev.shape[1] - 1]
        speech = {"net_input": {"source": torch.randn(B, S, generator=g).masked_fill(pm, 0.0), "padding_mask": pm, "prev_output_tokens": prev,
                                "tgt_lengths": dec_len // R, "spkembs": torch.randn(s["net_input"]["spkembs"].shape, generator=g)},
                  "target_list": [torch.randint(4, n_units, s["target_list"][0].shape, generator=g)],
                  "labels": (fr >= dec_len[:, None] - 1).float(), "dec_target": dec, "dec_target_lengths": dec_len,
                  "src_lengths": SRC_LEN[k], "id": s["id"].index_select(0, perm), "task_name": "speech_pretrain"}
        assert prev.shape[1] == L // R and speech["labels"].shape == s["labels"].shape
        Bt = t["target"].shape[0]
        perm = torch.randperm(Bt, generator=g)
        tgt = t["target"].index_select(0, perm)
        tgt = torch.where(tgt > 3, torch.randint(4, n_text, tgt.shape, generator=g), tgt)
        src = t["net_input"]["src_tokens"].index_select(0, perm)
        src = torch.where(src > 3, torch.randint(4, n_text, src.shape, generator=g), src)
        prv = torch.full_like(tgt, 1)
        for b in range(Bt):      # the row's last token moved to the front (collate_tokens, move_eos_to_beginning)
            nb = int((tgt[b] != 1).sum())
            prv[b, 0], prv[b, 1:nb] = tgt[b, nb - 1], tgt[b, :nb - 1]
        text = {"net_input": {"src_tokens": src, "src_lengths": t["net_input"]["src_lengths"].index_select(0, perm), "prev_output_tokens": prv},
                "target": tgt, "ntokens": int((tgt != 1).sum()), "id": t["id"].index_select(0, perm), "task_name": "text_pretrain"}
        assert text["ntokens"] == t["ntokens"]
        out.append([to_dev(speech, cuda), to_dev(text, cuda)])
    return out


class _Counted:
    def __init__(self, items):
        self.items, self.n = list(items), 0

    def __iter__(self):
        for it in self.items:
            self.n += 1
            yield it


def _run(cuda, mode, source, *, micro="side_by_side", prefetch=True, n_updates=5, after_update=None):
    """mode "eager": the static-shape eager update; "graph": two recording steps, capture, replays.  source: list of pairs or None
    (no set_source: the constructor's pair every time).  Returns (state, pulls, the update's static pair)."""
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
    try:
        static = [to_dev(fx_s["sample"], cuda), to_dev(fx_t["sample"], cuda)]
        upd = PretrainUpdate(task, model, crit, static, lr=1e-3, clip_norm=1.0, graph=mode == "graph", micro=micro,
                             prefetch_host=prefetch, device=cuda)
        src = None
        if source is not None:
            src = _Counted(source)
            upd.set_source(src)
        if mode == "graph":
            upd.prepare_graph()
            for k in range(2, n_updates):
                upd.update()
                if after_update is not None:
                    after_update(upd, k)
            if source is not None and len(source) == n_updates:
                with pytest.raises(StopIteration):       # the source has ended: the following update raises ...
                    upd.update()
                with pytest.raises(StopIteration):
                    upd.update()
            upd.finish()
        else:
            Fn._S.force_static = True
            for _ in range(n_updates):
                upd.eager_update()
            if source is not None and len(source) == n_updates:
                with pytest.raises(StopIteration):
                    upd.eager_update()
        state = upd.state()          # (... and ran nothing: the step count below is n_updates)
        return state, (src.n if src is not None else 0), static
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
    """Each reference run once, shared by the tests, never modified."""
    if key not in _cache:
        if key == "pairs":
            _cache[key] = _pairs(cuda)
        elif key == "eager_fed":
            _cache[key] = _run(cuda, "eager", _shared(cuda, "pairs"), micro="in_turn")
        elif key == "graph_no_source":
            _cache[key] = _run(cuda, "graph", None)
    return _cache[key]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _assert_state_equal(ref, got, what):
    assert ref[3] == got[3] == 5 and torch.isfinite(got[0]).all(), (what, ref[3], got[3])
    for x, y, name in zip(ref[:3], got[:3], ("parameters", "first moment", "second moment")):
        assert _same(x, y), (what, name, float((x - y).abs().max()))


@pytest.mark.parametrize("prefetch", [True, False], ids=["prefetch", "no_prefetch"])
@pytest.mark.parametrize("micro", ["in_turn", "side_by_side"])
def test_fed_replay_equals_eager_static(cuda, micro, prefetch):
    pairs = _shared(cuda, "pairs")
    ref, ref_pulls, _ = _shared(cuda, "eager_fed")
    got, pulls, static = _run(cuda, "graph", pairs, micro=micro, prefetch=prefetch)
    assert ref_pulls == 5 and pulls == 5          # every batch pulled once, none beyond the five trained on
    _assert_state_equal(ref, got, f"{micro}, prefetch={prefetch}")
    # after the last replay the static inputs (the constructor's tensors) hold the LAST batch of the source
    assert _same(static[0]["net_input"]["source"], pairs[4][0]["net_input"]["source"])
    assert _same(static[1]["target"], pairs[4][1]["target"]) and static[0]["src_lengths"] == SRC_LEN[4]


def test_feeding_the_recorded_pair_equals_the_replay_without_a_source(cuda):
    """Nothing changed for an update without a source: the load of the constructor's own data in front of every step is the only
    difference between the two runs, and the results are the same bits."""
    _, fx_s = load_golden("tiny_speech_pretrain.pt")
    _, fx_t = load_golden("tiny_text_pretrain.pt")
    same = [[to_dev(fx_s["sample"], cuda), to_dev(fx_t["sample"], cuda)] for _ in range(5)]
    ref, _, _ = _shared(cuda, "graph_no_source")
    got, pulls, _ = _run(cuda, "graph", same)
    assert pulls == 5
    _assert_state_equal(ref, got, "the recorded pair fed five times")


def test_the_fed_data_reaches_the_step(cuda):
    fed, _, _ = _shared(cuda, "eager_fed")
    alone, _, _ = _shared(cuda, "graph_no_source")
    assert fed[3] == alone[3] == 5 and not _same(fed[0], alone[0])


def test_span_mask_follows_the_current_batch_padding(cuda):
    """The stale-mirror case: pairs 3 and 4 -- two replayed updates -- pad different rows.  The span mask staged for a replayed update
    masks no frame inside THAT update's padding, while each of the two masks does reach into the other update's padding (a producer
    that kept the recorded step's mirror, pair 1's or none, could not pass both)."""
    pairs = _shared(cuda, "pairs")
    seen = {}

    def frame_pad(k, T):
        n = torch.tensor(SRC_LEN[k])
        pm = torch.arange(6000)[None, :] >= n[:, None]
        pm = pm[:, :6000 - 6000 % T]
        return pm.view(2, T, -1).all(-1)

    def look(upd, k):
        torch.cuda.synchronize()
        masks = [e[0] for e in upd.sg.staging.entries if e[0] is not None and e[0].dtype == torch.bool and e[0].dim() == 2 and e[0].shape[0] == 2]
        assert len(masks) == 1, [tuple(m.shape) for m in masks]
        seen[k] = masks[0].cpu().clone()
    _run(cuda, "graph", pairs, prefetch=True, after_update=look)
    assert sorted(seen) == [2, 3, 4]
    T = seen[3].shape[1]
    for k in (2, 3, 4):
        assert seen[k].any() and not (seen[k] & frame_pad(k, T)).any(), (k, seen[k].int().tolist())
    assert (seen[3] & frame_pad(4, T)).any() and (seen[4] & frame_pad(3, T)).any(), "the two paddings do not tell the mirrors apart"
