"""update.PretrainUpdate(stats=True) on the GPU (tiny model, bf16, dropout 0.1, LayerDrop 0.05, loss_weights [10, 0.1], clip 1.0): seven
updates -- two recorded, five replayed -- with a ring of four rows, so the ring wraps and three ring copies happen before the final one.
Every logged value the replayed update hands out through logging_outputs() is compared with `==` against an eager update that knows
nothing of the recorder: PretrainUpdate(graph=False, stats=False) around a criterion wrapped in a spy, whose returned tensors are read
with .item() after a synchronisation.  fp32 -> fp64 is exact on both sides and the replayed update is bit-equal to the eager one
(tests/test_batch_feed_gpu.py), so no tolerance applies."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from speecht5_amd import functional as Fn
from tests.util import Task, load_golden, to_dev

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N_UPDATES, ROWS, CLIP = 7, 4, 1.0
# speech rows' valid samples and log-mel frames per pair: pairs 1, 3 and 4 are right-padded, each differently
SRC_LEN = [[6000, 6000], [6000, 4200], [6000, 6000], [2400, 6000], [6000, 3000], [6000, 6000], [6000, 6000]]
DEC_LEN = [[24, 24], [24, 16], [24, 24], [10, 24], [24, 12], [24, 24], [24, 24]]
R = 2    # the tiny model's reduction factor


def _lr(n):
    return 1e-3 * (1.0 + 0.125 * n)      # another learning rate for every update


def _pairs(cuda, n=N_UPDATES):
    """Seven (speech, text) pairs in the fixtures' shapes, built as tests/test_batch_feed_gpu.py builds its five: waveforms and speaker
    embeddings re-drawn, unit labels and text tokens re-drawn inside their dictionaries, rows permuted; padded speech rows as the
    collater builds them."""
    _, fx_s = load_golden("tiny_speech_pretrain.pt")
    _, fx_t = load_golden("tiny_text_pretrain.pt")
    g = torch.Generator().manual_seed(4321)
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


class _Spy:
    """Forwards to the criterion and keeps what each call returned (the tensors stay referenced, so nothing reuses their memory)."""

    def __init__(self, crit):
        self.crit, self.calls = crit, []

    def __call__(self, model, sample, *a, **kw):
        out = self.crit(model, sample, *a, **kw)
        self.calls.append((sample["task_name"], out))
        return out


def _read_spy(calls):
    """The aggregated logging outputs train_step(sync=True) would have returned for these criterion calls, read with .item()."""
    aggs = []
    for name, (loss, sample_size, log) in calls:
        host = {k: (v.item() if torch.is_tensor(v) else v) for k, v in log.items()}
        agg = {"sample_size": 1, name: host}
        for k in ("ntokens", "nsentences"):
            if k in host:
                agg[k] = host[k]
        agg["loss"] = (loss.detach() / sample_size).item()
        aggs.append(agg)
    return aggs


def _pretrain_parts(cuda):
    from speecht5_amd.criterions import SpeechT5Criterion
    from speecht5_amd.speecht5 import T5TransformerModel
    from speecht5_amd.task import SpeechT5Task
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
    static = [to_dev(fx_s["sample"], cuda), to_dev(fx_t["sample"], cuda)]
    return task, model, crit, static


def _t2s_parts(cuda):
    """One fine-tuning criterion: the t2s fixture with guided attention on (fp32, the fused loss kernels), one micro-batch."""
    from speecht5_amd.criterions import SpeechT5Criterion
    from speecht5_amd.speecht5 import T5TransformerModel
    from speecht5_amd.task import SpeechT5Task
    m, fx = load_golden("tiny_t2s.pt")
    args = Namespace(**m["args"])
    Fn.set_compute_dtype(torch.float32)
    task = SpeechT5Task(args, Task().dicts)
    model = T5TransformerModel.build_model(args, task)
    torch.nn.Module.load_state_dict(model, m["state_dict"], strict=True)
    model.use_codebook = False
    model = model.to(cuda).train()
    crit = SpeechT5Criterion(task, use_guided_attn_loss=True, guided_attn_loss_sigma=0.4, guided_attn_loss_lambda=10.0, sync_logging=False)
    return task, model, crit, [to_dev(fx["sample"], cuda)]


def _cleanup(upd):
    Fn._S.force_static = False
    if upd is not None:
        upd.close()
    Fn.bf16_mirror.__init__()
    Fn.weight_cache.clear()
    Fn.set_layer_boundary_hook(None)
    Fn.set_compute_dtype(torch.float32)


def _seed():
    Fn.manual_seed(21)
    np.random.seed(8)
    torch.manual_seed(8)


def _eager_spy(cuda, parts, source, n_updates=N_UPDATES):
    """The reference arm: graph=False, stats=False, static shapes, the criterion behind a spy; after every update a synchronisation and
    one .item() per logged tensor."""
    from speecht5_amd.update import PretrainUpdate
    task, model, crit, static = parts(cuda)
    spy = _Spy(crit)
    _seed()
    upd = None
    try:
        upd = PretrainUpdate(task, model, spy, static, lr=1e-3, clip_norm=CLIP, graph=False, micro="in_turn", device=cuda, lr_fn=_lr)
        if source is not None:
            upd.set_source(list(source))
        Fn._S.force_static = True
        out = []
        for _ in range(n_updates):
            spy.calls = []
            upd.eager_update()
            torch.cuda.synchronize()
            assert len(spy.calls) == len(static)
            gsq = float(upd.opt.gnorm_sq)
            gnorm = math.sqrt(gsq) / len(static)
            out.append({"num_updates": upd.n, "lr": float(upd.opt.lr), "gnorm_sq": gsq, "gnorm": gnorm, "clip": gnorm > CLIP,
                        "logging_outputs": _read_spy(spy.calls)})
        return out
    finally:
        _cleanup(upd)


def _replayed(cuda, parts, source, *, micro, prefetch, stats=True, n_updates=N_UPDATES):
    """Two recording updates, capture, n_updates - 2 replays; logging_outputs() between the updates.  -> (entries, state, notes)."""
    from speecht5_amd.update import PretrainUpdate
    task, model, crit, static = parts(cuda)
    _seed()
    upd = None
    try:
        upd = PretrainUpdate(task, model, crit, static, lr=1e-3, clip_norm=CLIP, graph=True, micro=micro, prefetch_host=prefetch, device=cuda,
                             lr_fn=_lr, stats=stats, stats_rows=ROWS)
        if source is not None:
            upd.set_source(list(source))
        entries, notes = [], {"waits": [], "copies": 0, "between": []}
        if stats:
            sched, where = upd.stats.sched, ["update"]
            wait, copy = sched.wait, sched.copy
            sched.wait = lambda ev: (notes["waits"].append(where[0]), wait(ev))[1]

            def counted(image):
                notes["copies"] += 1
                return copy(image)
            sched.copy = counted
        upd.prepare_graph()
        for k in range(2, n_updates):
            upd.update()
            if stats:
                where[0] = "logging_outputs"
                part = upd.logging_outputs()
                where[0] = "update"
                assert all(e["num_updates"] <= k + 1 for e in part)
                notes["between"].append(len(part))
                entries += part
        upd.finish()
        if stats:
            entries += upd.logging_outputs()
            assert upd.logging_outputs() == [] and upd.logging_outputs(wait=True) == []
        return entries, upd.state(), notes
    finally:
        _cleanup(upd)


_cache = {}


def _shared(cuda, key):
    """Each reference run once, shared by the tests, never modified."""
    if key not in _cache:
        if key == "pairs":
            _cache[key] = _pairs(cuda)
        elif key == "eager_static":
            _cache[key] = _eager_spy(cuda, _pretrain_parts, None)
        elif key == "eager_fed":
            _cache[key] = _eager_spy(cuda, _pretrain_parts, _shared(cuda, "pairs"))
        elif key == "replayed_fed_stats":
            _cache[key] = _replayed(cuda, _pretrain_parts, _shared(cuda, "pairs"), micro="side_by_side", prefetch=True)
    return _cache[key]


def _assert_entries_equal(ref, got, what):
    assert [e["num_updates"] for e in got] == list(range(1, len(ref) + 1)), (what, [e["num_updates"] for e in got])
    for r, g in zip(ref, got):
        n = r["num_updates"]
        assert set(g) == set(r), (what, n, set(g) ^ set(r))
        for k in ("num_updates", "lr", "gnorm_sq", "gnorm", "clip"):
            assert type(g[k]) is type(r[k]) and g[k] == r[k], (what, n, k, g[k], r[k])
        assert len(g["logging_outputs"]) == len(r["logging_outputs"])
        for i, (ra, ga) in enumerate(zip(r["logging_outputs"], g["logging_outputs"])):
            assert list(ga) == list(ra), (what, n, i, list(ga), list(ra))
            for k, rv in ra.items():
                if isinstance(rv, dict):
                    assert list(ga[k]) == list(rv), (what, n, i, k, list(ga[k]), list(rv))
                    for kk, rvv in rv.items():
                        assert type(ga[k][kk]) is type(rvv) and ga[k][kk] == rvv, (what, n, i, k, kk, ga[k][kk], rvv)
                else:
                    assert type(ga[k]) is type(rv) and ga[k] == rv, (what, n, i, k, ga[k], rv)


@pytest.mark.parametrize("fed", [False, True], ids=["constructor_pair", "seven_pairs"])
@pytest.mark.parametrize("prefetch", [True, False], ids=["prefetch", "no_prefetch"])
@pytest.mark.parametrize("micro", ["in_turn", "side_by_side"])
def test_replayed_logging_outputs_equal_the_eager_items(cuda, micro, prefetch, fed):
    ref = _shared(cuda, "eager_fed" if fed else "eager_static")
    if fed and micro == "side_by_side" and prefetch:
        got, _, notes = _shared(cuda, "replayed_fed_stats")
    else:
        got, _, notes = _replayed(cuda, _pretrain_parts, _shared(cuda, "pairs") if fed else None, micro=micro, prefetch=prefetch)
    what = f"{micro}, prefetch={prefetch}, fed={fed}"
    assert len(ref) == N_UPDATES and len(got) == N_UPDATES, (what, len(got))
    _assert_entries_equal(ref, got, what)
    # the logs really carry what the trainer reports, the values move from update to update, and the feed changes them
    first = got[0]["logging_outputs"]
    assert {"loss_m_0", "dec_loss", "l1_loss", "bce_loss", "loss_prob_perplexity", "code_perplexity", "sample_size", "loss"} <= set(first[0]["speech_pretrain"])
    assert {"bart_loss", "loss", "ntokens", "nsentences"} <= set(first[1]["text_pretrain"])
    assert len({e["logging_outputs"][1]["loss"] for e in got}) == N_UPDATES and len({e["lr"] for e in got}) == N_UPDATES
    assert all(e["gnorm_sq"] > 0 and e["gnorm"] == math.sqrt(e["gnorm_sq"]) * 0.5 and e["clip"] == (e["gnorm"] > CLIP) for e in got)
    # logging_outputs() between the updates never waited for the device; the ring was copied at updates 2, 4, 6 and once at the end
    assert "logging_outputs" not in notes["waits"], notes
    assert notes["copies"] == 4, notes


def test_the_feed_changes_what_is_logged(cuda):
    a, b = _shared(cuda, "eager_static"), _shared(cuda, "eager_fed")
    assert a[0]["logging_outputs"][0]["loss"] != b[0]["logging_outputs"][0]["loss"] or a[2]["logging_outputs"][0]["loss"] != b[2]["logging_outputs"][0]["loss"]


def test_stats_do_not_change_the_update(cuda):
    """state() after seven replayed updates, side by side, fed: the same bits with and without the recorder."""
    _, with_stats, _ = _shared(cuda, "replayed_fed_stats")
    _, without, _ = _replayed(cuda, _pretrain_parts, _shared(cuda, "pairs"), micro="side_by_side", prefetch=True, stats=False)
    assert with_stats[3] == without[3] == N_UPDATES and torch.isfinite(with_stats[0]).all()
    for x, y, name in zip(with_stats[:3], without[:3], ("parameters", "first moment", "second moment")):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32)), name


def test_fine_tuning_criterion_keys_and_types(cuda):
    """t2s with guided attention, one micro-batch, in turn, replayed, against its eager spy: keys the pre-training logs do not have
    (enc_dec_attn_loss, the scaled positional encodings' alphas -- parameters, read behind Adam on both sides)."""
    ref = _eager_spy(cuda, _t2s_parts, None, n_updates=5)
    got, _, _ = _replayed(cuda, _t2s_parts, None, micro="in_turn", prefetch=True, n_updates=5)
    _assert_entries_equal(ref, got, "t2s")
    log = got[-1]["logging_outputs"][0]["t2s"]
    assert {"enc_dec_attn_loss", "encoder_alpha", "decoder_alpha", "l1_loss", "l2_loss", "bce_loss"} <= set(log)
    assert isinstance(log["enc_dec_attn_loss"], float) and log["ntokens"] == 61 and log["nsentences"] == 3


def test_reduce_metrics_takes_the_harvested_entries(cuda):
    from speecht5_amd import fairseq_compat as fc
    from speecht5_amd.criterions import SpeechT5Criterion
    assert not fc.HAVE_FAIRSEQ
    ref = _shared(cuda, "eager_fed")
    got, _, _ = _shared(cuda, "replayed_fed_stats")
    for n in (0, 4, 6):        # a recorded update and two replayed ones
        calls = []
        for entry in (ref[n], got[n]):
            fc.metrics.reset()
            SpeechT5Criterion.reduce_metrics(entry["logging_outputs"])
            derived = {k: fn(fc.metrics.meters) for k, fn in fc.metrics.derived.items()}
            calls.append(([list(c) for c in fc.metrics.recorded], derived))
        assert calls[0][0] == calls[1][0] and len(calls[0][0]) > 10, n
        assert calls[0][1].keys() == calls[1][1].keys() and all(calls[0][1][k] == calls[1][1][k] for k in calls[0][1]), n
        names = [c[1] for c in calls[1][0]]
        assert {"hubert_loss", "hubert_loss_m_0", "hubert_dec_loss", "hubert_code_perplexity", "text_loss", "bart_loss", "loss"} <= set(names), names
    fc.metrics.reset()


class _TwoElements:
    def __init__(self, crit):
        self.crit, self.sync_logging = crit, False

    def __call__(self, model, sample, *a, **kw):
        loss, n, log = self.crit(model, sample, *a, **kw)
        if sample["task_name"] == "text_pretrain":
            log["pair"] = torch.stack([log["loss"], log["bart_loss"]])
        return loss, n, log


def test_refusals(cuda):
    from speecht5_amd.criterions import SpeechT5Criterion
    from speecht5_amd.update import PretrainUpdate
    task, model, crit, static = _pretrain_parts(cuda)
    upd = None
    try:
        _seed()
        # a two-element tensor under a logging key: refused by key path at the first update
        upd = PretrainUpdate(task, model, _TwoElements(crit), static, lr=1e-3, clip_norm=CLIP, graph=False, micro="in_turn", device=cuda, stats=True)
        Fn._S.force_static = True
        with pytest.raises(ValueError, match=r"micro\[1\]\.text_pretrain\.pair"):
            upd.eager_update()
        torch.cuda.synchronize()
        upd.close()
        upd = None
        Fn._S.force_static = False
        # host floats from the criterion cannot be captured
        sync_crit = SpeechT5Criterion(task, loss_weights=[10, 0.1], sync_logging=True)
        with pytest.raises(ValueError, match="sync_logging"):
            PretrainUpdate(task, model, sync_crit, static, lr=1e-3, clip_norm=CLIP, graph=True, device=cuda, stats=True)
        with pytest.raises(ValueError, match="at least 2 rows"):
            PretrainUpdate(task, model, crit, static, lr=1e-3, clip_norm=CLIP, graph=True, device=cuda, stats=True, stats_rows=1)
    finally:
        _cleanup(upd)


def test_logging_outputs_without_stats_raises(cuda):
    from speecht5_amd.update import PretrainUpdate
    task, model, crit, static = _pretrain_parts(cuda)
    upd = None
    try:
        upd = PretrainUpdate(task, model, crit, static, lr=1e-3, clip_norm=CLIP, graph=False, device=cuda)
        assert upd.stats is None
        with pytest.raises(RuntimeError, match="stats=False"):
            upd.logging_outputs()
    finally:
        _cleanup(upd)
