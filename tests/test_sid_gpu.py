"""Speaker identification (t5_task s2c) on the HIP path: tiny whole-model parity with the verbatim reference (tests/golden/tiny_s2c.pt,
tools/make_golden_sid.py), the margin and time-mean kernels against fp64 at recipe shapes, a Base-size recipe training step in bf16
against fp32, generate_class on a 160 s utterance, and the class collater against the reference's."""
import math
import os
from argparse import Namespace

import pytest
import torch

from tests import sid_reference as R
from tests.util import G, close, to_dev

pytestmark = pytest.mark.gpu

CASES = ["recipe", "default", "normalize", "amsoftmax", "aamsoftmax", "aamsoftmax_easy", "encoder", "encoder_cls"]


@pytest.fixture(scope="module")
def fx():
    return torch.load(os.path.join(G, "tiny_s2c.pt"), weights_only=False)


class SidTask:
    def __init__(self, n_spk):
        from tests.util import Dictionary
        self.dicts = {"text": Dictionary(n_spk, ["<mask>", "<ctc_blank>"])}
        self.t5_task = "s2c"
        self.target_dictionary = self.dicts["text"]
        self.blank_symbol_idx = self.dicts["text"].index("<ctc_blank>")


def _tiny(fx, name, dev, dtype):
    from speecht5_amd import functional as Fn
    from speecht5_amd.speecht5 import T5TransformerModel
    Fn.set_compute_dtype(dtype)
    Fn.weight_cache.clear()    # (a fresh model may reuse a freed parameter's address: no transposed copy of the last case's)
    case = fx["cases"][name]
    model = T5TransformerModel.build_model(Namespace(**case["args"]), SidTask(fx["n_spk"]))
    tiny = torch.load(os.path.join(G, "tiny_model.pt"), weights_only=False)["state_dict"]
    sd = dict(model.state_dict())
    for k in fx["trunk_keys"]:
        sd[k] = tiny[k]
    sd.update(fx["shared_state"])
    sd.update(case["state"])
    torch.nn.Module.load_state_dict(model, {k: sd[k] for k in model.state_dict()}, strict=True)
    return model.to(dev)


def _sample(fx, name, dev):
    s = to_dev(fx["sample"], dev)
    s["net_input"] = dict(s["net_input"])
    if fx["cases"][name]["target_list"]:
        s["net_input"]["target_list"] = s["target"]
    return s


def _criterion(fx):
    from speecht5_amd.criterions import SpeechtoTextLoss
    return SpeechtoTextLoss(None, SidTask(fx["n_spk"]), sentence_avg=False, label_smoothing=0.1, report_accuracy=True, ce_weight=1.0,
                            ctc_weight=0.0)


@pytest.mark.parametrize("name", CASES)
def test_tiny_fp32_matches_reference(cuda, fx, name):
    case = fx["cases"][name]
    model = _tiny(fx, name, cuda, torch.float32)
    model.train()
    sample = _sample(fx, name, cuda)
    seen = {}
    hook = model.speaker_decoder_postnet.register_forward_hook(lambda m, i, o: seen.update(logits=o[0].detach().clone()))
    loss, ss, log = _criterion(fx)(model, sample)
    hook.remove()
    close(seen["logits"], case["train_logits"], 2e-4, what="train logits")
    close(loss, case["loss"], 2e-4, what="loss")
    assert ss == case["sample_size"]
    assert (log["n_correct"], log["total"]) == (case["log"]["n_correct"], case["log"]["total"])
    (loss / ss).backward()
    torch.cuda.synchronize()
    got = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    # With BatchNorm over B = 3 pooled rows the trunk's gradient is the batch-centred part of the head's: e.g. the decoder's last
    # LayerNorm bias gets sum_b dy_b = 0 exactly, and the reference's own fp32 values there are rounding noise (fp64 gives ~1e-17).
    # Every tensor is therefore held to 2e-3 of its own scale plus 1e-4 of the step's largest gradient norm.
    scale = max(case["grads"]["norms"].values())
    for n, ref in case["grads"]["norms"].items():
        g = float(got[n].double().norm()) if n in got else 0.0
        assert abs(g - ref) <= 2e-3 * ref + 1e-4 * scale, (n, g, ref)
    for n, ref in case["grads"]["full"].items():
        close(got[n], ref, 2e-3, what=f"grad {n}", floor=1e-4 * scale)
    for k, ref in case["bn_state"].items():
        v = model.state_dict()[k]
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref), k
        else:
            close(v, ref, 2e-4, what=k)
    model.eval()
    ni = sample["net_input"]
    with torch.no_grad():
        (logits, embed), _ = model(**ni)
        close(logits, case["eval_logits"], 2e-4, what="eval logits")
        close(embed, case["eval_embed"], 2e-4, what="eval embed")
        cls = model.generate_class(ni["source"], ni["prev_output_tokens"], padding_mask=ni["padding_mask"])
    assert cls.dtype == torch.int64 and torch.equal(cls.cpu(), case["classes"])


@pytest.mark.parametrize("name", ["recipe", "default", "aamsoftmax"])
def test_tiny_bf16_close_to_reference(cuda, fx, name):
    case = fx["cases"][name]
    try:
        model = _tiny(fx, name, cuda, torch.bfloat16)
        model.train()
        loss, ss, _ = _criterion(fx)(model, _sample(fx, name, cuda))
        close(loss, case["loss"], 6e-2, what="bf16 loss")
        (loss / ss).backward()
        model.eval()
        with torch.no_grad():
            (logits, embed), _ = model(**_sample(fx, name, cuda)["net_input"])
        close(logits, case["eval_logits"], 6e-2, what="bf16 eval logits")
    finally:
        from speecht5_amd import functional as Fn
        Fn.set_compute_dtype(torch.float32)


def test_task_generate_class(cuda, fx):
    from speecht5_amd.task import SpeechT5Task
    model = _tiny(fx, "default", cuda, torch.float32)
    model.eval()
    ni = to_dev(fx["sample"], cuda)["net_input"]
    cls = SpeechT5Task.generate_class(None, [model], ni, ni["prev_output_tokens"])
    assert torch.equal(cls.cpu(), fx["cases"]["default"]["classes"])


def test_batch_of_one_in_training_raises_like_batchnorm(cuda, fx):
    model = _tiny(fx, "default", cuda, torch.float32)
    model.train()
    ni = to_dev(fx["sample"], cuda)["net_input"]
    one = dict(ni, source=ni["source"][:1], padding_mask=ni["padding_mask"][:1], prev_output_tokens=ni["prev_output_tokens"][:1])
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        model(**one)


# ---- kernels vs fp64 at recipe shapes ----
def _err(a, b):
    return (a.double() - b.double()).abs().max().item()


def _margin_inputs(B, V, m, dev, seed):
    g = torch.Generator().manual_seed(seed)
    cos = (torch.rand(B, V, generator=g) * 2 - 1) * 0.9
    target = torch.randint(4, V, (B,), generator=g)
    th = math.cos(math.pi - m)
    cos[0, target[0]] = 1.0
    cos[1, target[1]] = -1.0
    cos[2, target[2]] = th                                          # at th (rounded to fp32)
    cos[3, target[3]] = torch.nextafter(torch.tensor(th, dtype=torch.float32), torch.tensor(1.0)).item()
    cos[4, target[4]] = 0.9999999
    cos[5, target[5]] = -0.9999
    cos[6, :] = torch.linspace(-1, 1, V)
    target[B - 1] = -1                                              # no margin in the last row
    return cos, target


@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("mode", [R.MARGIN_AM, R.MARGIN_AAM, R.MARGIN_AAM_EASY])
@pytest.mark.parametrize("m,s", [(0.0, 1.0), (0.2, 1.0), (0.2, 30.0), (0.0, 30.0)])
def test_margin_kernels_match_fp64(cuda, B, mode, m, s):
    from speecht5_amd import hip
    V = 1257
    ld = (V + 3) // 4 * 4
    cos, target = _margin_inputs(B, V, m, cuda, seed=B * 10 + mode)
    dy = torch.randn(B, V, generator=torch.Generator().manual_seed(7))
    c_dev = torch.full((B, ld), float("nan"), device=cuda)
    c_dev[:, :V] = cos.to(cuda)
    t_dev = target.to(torch.int32).to(cuda)
    out = torch.full((B, ld), float("nan"), device=cuda)
    L = hip.lib()
    hip.check(L.st5_angular_margin_fwd(c_dev.data_ptr(), ld, t_dev.data_ptr(), out.data_ptr(), ld, B, V, mode, m, s, hip.stream()), "fwd")
    dy_dev = torch.full((B, ld + 4), float("nan"), device=cuda)
    dy_dev[:, :V] = dy.to(cuda)
    dc = torch.full((B, ld), float("nan"), device=cuda)
    hip.check(L.st5_angular_margin_bwd(c_dev.data_ptr(), ld, t_dev.data_ptr(), dy_dev.data_ptr(), ld + 4, dc.data_ptr(), ld, B, V, mode,
                                       m, s, hip.stream()), "bwd")
    torch.cuda.synchronize()
    out, dc = out.cpu(), dc.cpu()
    assert torch.isnan(out[:, V:]).all()                            # columns past V untouched
    assert (dc[:, V:] == 0).all()                                   # padded gradient columns zeroed
    ref = R.margin(cos, target, mode, m, s)
    t32 = R.margin(cos, target, mode, m, s, dtype=torch.float32)
    assert torch.isfinite(out[:, :V]).all()
    assert _err(out[:, :V], ref) <= 4 * _err(t32, ref) + 1e-7 * s
    gref = R.margin_grad(cos, target, dy, mode, m, s)
    g32 = R.margin_grad(cos, target, dy, mode, m, s, dtype=torch.float32)
    assert torch.isfinite(dc[:, :V]).all()
    assert _err(dc[:, :V], gref) <= 4 * _err(g32, gref) + 1e-6 * s


@pytest.mark.parametrize("T,B", [(159, 8), (8000, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_time_mean_kernels_match_fp64(cuda, T, B, dtype):
    from speecht5_amd import functional as Fn
    C = 768
    g = torch.Generator().manual_seed(T + B)
    x = (torch.randn(T, B, C, generator=g) * 2 + 0.5).to(dtype)
    ref = x.double().mean(0)
    t32 = x.float().mean(0)
    xd = x.to(cuda).requires_grad_(True)
    y = Fn.time_mean(xd)
    dy = torch.randn(B, C, generator=g)
    y.backward(dy.to(cuda))
    torch.cuda.synchronize()
    assert y.dtype == torch.float32
    assert _err(y.cpu(), ref) <= 4 * _err(t32, ref) + 1e-9
    gref = (dy.double() / T).expand(T, B, C)
    g32 = (dy / T).to(dtype).expand(T, B, C)
    assert _err(xd.grad.cpu(), gref) <= 4 * _err(g32, gref) + 1e-12
    # a batch-major [B, T, C] tensor seen time-major (the decoder output's mean(1)): strides, no copy
    xb = x.transpose(0, 1).contiguous().to(cuda)
    assert _err(Fn.time_mean(xb.transpose(0, 1)).cpu(), ref) <= 4 * _err(t32, ref) + 1e-9


# ---- recipe shapes at Base size ----
def _base(cuda, dtype, n_spk=1251, **over):
    from speecht5_amd import functional as Fn
    from speecht5_amd.speecht5 import t5_transformer_base_asr
    from speecht5_amd.task import SpeechT5Task, _Dictionary
    Fn.set_compute_dtype(dtype)
    Fn.weight_cache.clear()
    args = Namespace(label_rates=50, sample_rate=16000, speech_odim=80, bert_init=True, use_codebook=False, share_input_output_embed=True,
                     encoder_layerdrop=0.0, decoder_layerdrop=0.0, mask_prob=0.0, mask_channel_prob=0.0, feature_grad_mult=1.0,
                     relative_position_embedding=True, sid_no_pooling_bn=True, sid_no_embed_postnet=True, t5_task="s2c", **over)
    t5_transformer_base_asr(args)
    for k, v in list(vars(args).items()):
        if "dropout" in k and isinstance(v, float):
            setattr(args, k, 0.0)
    task = SpeechT5Task(args, {"text": _Dictionary([f"id{i}" for i in range(n_spk)])})
    torch.manual_seed(1234)
    model = task.build_model(args)
    return task, model.to(cuda), args


def _recipe_batch(B, S, n_cls, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(net_input=dict(source=torch.randn(B, S, generator=g), padding_mask=torch.zeros(B, S, dtype=torch.bool),
                               prev_output_tokens=torch.full((B, 1), 2, dtype=torch.long), task_name="s2c"),
                target=torch.randint(4, n_cls - 2, (B, 1), generator=g), target_lengths=torch.ones(B, dtype=torch.long), ntokens=B,
                task_name="s2c", id=torch.arange(B))


def test_base_recipe_step_bf16_close_to_fp32_and_reports_accuracy(cuda):
    """The SID recipe's update at Base size: 8 x 51,200 samples (159 frames), class_num 1257, softmax head, through the task's
    train_step and the speecht5 criterion; s2c_accuracy comes out of reduce_metrics."""
    from speecht5_amd import fairseq_compat as fc
    from speecht5_amd import functional as Fn
    from speecht5_amd.criterions import SpeechT5Criterion
    res = {}
    try:
        for dtype in (torch.float32, torch.bfloat16):
            task, model, args = _base(cuda, dtype)
            assert model.speaker_decoder_postnet.class_num == 1257
            sample = to_dev(_recipe_batch(8, 51200, 1257, seed=5), cuda)
            crit = SpeechT5Criterion(task, report_accuracy=True)
            loss, _, agg = task.train_step(sample, model, crit, None, 0)
            torch.cuda.synchronize()
            head = model.speaker_decoder_postnet.output_projection.weight.grad.detach().double().cpu()
            enc = model.encoder.layers[0].fc1.weight.grad.detach().double().cpu()
            res[dtype] = (loss, agg, head, enc)
            del model
    finally:
        Fn.set_compute_dtype(torch.float32)
    (l32, a32, h32, e32), (l16, a16, h16, e16) = res[torch.float32], res[torch.bfloat16]
    assert math.isfinite(l32) and abs(l16 - l32) <= 2e-2 * abs(l32), (l16, l32)
    for a, b in ((h16, h32), (e16, e32)):
        cosim = float((a * b).sum() / (a.norm() * b.norm()))
        assert cosim > 0.98, cosim
    log = a32["s2c"]
    assert log["total"] == 8 and 0 <= log["n_correct"] <= 8
    fc.metrics.reset()
    SpeechT5Criterion.reduce_metrics([a32])
    vals = fc.metrics.get_smoothed_values()
    assert vals["s2c_accuracy"] == round(log["n_correct"] * 100.0 / 8, 3)


def _classify(cuda, dtype, wav):
    task, model, args = _base(cuda, dtype)
    model.eval()
    S = wav.shape[1]
    ni = dict(source=wav.to(cuda), padding_mask=torch.zeros(1, S, dtype=torch.bool, device=cuda),
              prev_output_tokens=torch.full((1, 1), 2, dtype=torch.long, device=cuda))
    cls = task.generate_class([model], dict(ni, task_name="s2c"), ni["prev_output_tokens"])
    with torch.no_grad():
        (logits, _), _ = model(**ni, task_name="s2c")
    torch.cuda.synchronize()
    assert cls.shape == (1,) and cls.dtype == torch.int64
    assert torch.isfinite(logits).all()
    assert int(cls) == int(logits.argmax(1))
    return logits.double().cpu()


def test_generate_class_160s_utterance(cuda):
    """generate_class as scripts/generate_class.py runs it: batch 1, a whole test utterance at the length cap of the recipe's test splits
    (2,560,000 samples = 160 s, 7999 encoder frames; one decoder query against them).  bf16 completes on the flash-attention kernels.
    fp32 attention is the unfused path, which takes at most 4096 keys (81.9 s): it refuses with a clear error; bf16 and fp32 logits
    are compared at 60 s."""
    from speecht5_amd import functional as Fn
    g = torch.Generator().manual_seed(11)
    wav = torch.randn(1, 2_560_000, generator=g) * 0.1
    try:
        _classify(cuda, torch.bfloat16, wav)
        with pytest.raises(ValueError, match="at most 4096 keys"):
            _classify(cuda, torch.float32, wav)
        short = wav[:, :960_000].contiguous()
        close(_classify(cuda, torch.bfloat16, short), _classify(cuda, torch.float32, short), 6e-2, what="bf16 vs fp32 logits at 60 s")
    finally:
        Fn.set_compute_dtype(torch.float32)


def test_class_collater_bit_identical_to_reference(cuda, fx):
    from speecht5_amd.collate import SpeechToClassCollater
    col = fx["collate"]
    items = [{k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in it.items()} for it in col["items"]]
    got = SpeechToClassCollater(cuda)(items)
    ref = col["batch"]
    for k in ("source", "padding_mask", "prev_output_tokens"):
        a, b = got["net_input"][k].cpu(), ref["net_input"][k]
        assert a.dtype == b.dtype and torch.equal(a, b), k
    assert got["net_input"]["task_name"] == ref["net_input"]["task_name"] == "s2c"
    for k in ("target", "target_lengths", "id"):
        a, b = got[k].cpu(), ref[k]
        assert a.dtype == b.dtype and torch.equal(a, b), k
    assert got["ntokens"] == ref["ntokens"] and got["task_name"] == ref["task_name"]


class _FixedLogits(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward(self, **kw):
        return (self.logits, None), None


def test_s2t_accuracy_skips_pad_targets(cuda):
    """report_accuracy on s2t: argmax hits over non-pad targets only; off, the logging output is what it was."""
    from speecht5_amd.criterions import SpeechtoTextLoss
    from tests.util import Task
    g = torch.Generator().manual_seed(2)
    V = 36
    logits = torch.randn(2, 5, V, generator=g)
    target = logits.argmax(-1)
    target[0, 1] = 5 if int(target[0, 1]) != 5 else 6                              # one miss
    target[1, 3:] = 1                                                                # pad (where the argmax may or may not be 1)
    logits[1, 3, 1] = 50.0                                                           # a pad position whose argmax IS the pad id
    sample = dict(net_input={}, target=target.to(cuda), ntokens=8, task_name="s2t")
    model = _FixedLogits(logits.to(cuda))
    crit = SpeechtoTextLoss(None, Task(), sentence_avg=False, label_smoothing=0.1, report_accuracy=True)
    _, _, log = crit(model, dict(sample))
    mask = target.ne(1)
    want = int((logits.argmax(-1).eq(target) & mask).sum())
    assert (log["n_correct"], log["total"]) == (want, int(mask.sum()))
    _, _, log0 = SpeechtoTextLoss(None, Task(), sentence_avg=False, label_smoothing=0.1)(model, dict(sample))
    assert "n_correct" not in log0 and "total" not in log0
