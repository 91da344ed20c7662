"""CPU checks of the speaker-identification (s2c) layer: the fp64 restatement in tests/sid_reference.py against the reference fixture
(tests/golden/tiny_s2c.pt, tools/make_golden_sid.py) and torch, the refused options, the head's state-dict keys, and a scratch-free
build of csrc/speaker_head.hip."""
import os
import sys
from argparse import Namespace

import pytest
import torch

from tests import sid_reference as R
from tests.util import G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _head_sd(case):
    p = "speaker_decoder_postnet."
    return {k[len(p):]: v for k, v in case["state"].items() if k.startswith(p)}


def _target(fx):
    return fx["sample"]["target"][:, 0]


@pytest.mark.parametrize("name", ["recipe", "aamsoftmax", "aamsoftmax_easy", "encoder"])
def test_head_restatement_matches_reference(fx, name):
    """Heads without BatchNorm: the eval embed IS the pooled input, so eval and train logits follow from it alone."""
    case = fx["cases"][name]
    args = Namespace(**case["args"])
    sd = _head_sd(case)
    pooled = case["eval_embed"]
    ev, emb = R.head(pooled, sd, args, training=False)
    torch.testing.assert_close(ev, case["eval_logits"].double(), rtol=0, atol=2e-5 * case["eval_logits"].abs().max().item())
    tr, _ = R.head(pooled, sd, args, training=True, target=_target(fx) if case["target_list"] else None)
    torch.testing.assert_close(tr, case["train_logits"].double(), rtol=0, atol=2e-5 * case["train_logits"].abs().max().item())


def test_margin_cases_cover_both_branches(fx):
    th = torch.cos(torch.tensor(torch.pi - 0.2, dtype=torch.float64))
    c = fx["cases"]["aamsoftmax"]["eval_logits"].double().gather(1, fx["sample"]["target"]).squeeze(1)
    assert (c < th).any() and (c > th).any() and (c > 0).any() and (c <= 0).any()


def test_margin_grad_is_autograd_of_margin():
    g = torch.Generator().manual_seed(0)
    cos = (torch.rand(6, 37, generator=g, dtype=torch.float64) * 2 - 1) * 0.999
    cos[0, 3] = -0.9995          # below th of m = 0.2
    cos[1, 5] = 0.9995
    target = torch.tensor([3, 5, -1, 0, 36, 7])
    dy = torch.randn(6, 37, generator=g, dtype=torch.float64)
    for mode in (R.MARGIN_AM, R.MARGIN_AAM, R.MARGIN_AAM_EASY):
        for m, s in ((0.2, 30.0), (0.0, 1.0), (0.5, 2.0)):
            x = cos.clone().requires_grad_(True)
            R.margin(x, target, mode, m, s).backward(dy)
            torch.testing.assert_close(R.margin_grad(cos, target, dy, mode, m, s), x.grad, rtol=1e-12, atol=1e-12)


def test_margin_grad_finite_at_unit_cosine():
    cos = torch.tensor([[1.0, 0.3], [-1.0, 0.3]], dtype=torch.float64)
    g = R.margin_grad(cos, torch.tensor([0, 0]), torch.ones_like(cos), R.MARGIN_AAM, 0.2, 30.0)
    assert torch.isfinite(g).all()
    assert abs(g[0, 0].item() - 30.0 * torch.cos(torch.tensor(0.2, dtype=torch.float64)).item()) < 1e-12   # phi branch
    assert g[1, 0].item() == 30.0                                                                            # cos - mm branch


@pytest.mark.parametrize("training", [True, False])
def test_batch_norm_restatement_matches_torch(training):
    g = torch.Generator().manual_seed(1)
    bn = torch.nn.BatchNorm1d(12).double()
    with torch.no_grad():
        bn.weight.normal_(generator=g)
        bn.bias.normal_(generator=g)
        bn.running_mean.normal_(generator=g)
        bn.running_var.uniform_(0.5, 2.0, generator=g)
    x = torch.randn(5, 12, generator=g, dtype=torch.float64)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn.train(training)
    y = bn(x)
    y2, rm, rv = R.batch_norm(x, bn.weight, bn.bias, rm0, rv0, training)
    torch.testing.assert_close(y2, y.detach())
    torch.testing.assert_close(rm, bn.running_mean)
    torch.testing.assert_close(rv, bn.running_var)


def _build(fx, name, **over):
    from speecht5_amd.speecht5 import T5TransformerModel
    args = Namespace(**fx["cases"][name]["args"])
    for k, v in over.items():
        setattr(args, k, v)
    return T5TransformerModel.build_model(args, SidTask(fx["n_spk"]))


@pytest.mark.parametrize("name", ["recipe", "default", "amsoftmax", "encoder_cls"])
def test_state_dict_keys_round_trip(fx, name):
    model = _build(fx, name)
    case = fx["cases"][name]
    head = [k for k in case["state_keys"] if k.startswith("speaker_decoder_postnet.")]
    ours = [k for k in model.state_dict() if k.startswith("speaker_decoder_postnet.")]
    assert ours == head
    assert set(case["state_keys"]) <= set(model.state_dict()) | {k for k in case["state_keys"] if k.endswith("_float_tensor")}
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd.update(case["state"])
    model.load_state_dict(sd)
    for k, v in case["state"].items():
        assert torch.equal(model.state_dict()[k], v), k


@pytest.mark.parametrize("over,word", [
    (dict(sid_pooling_layer="decoder-las"), "decoder-las"),
    (dict(sid_pooling_layer="encoder-speaker"), "encoder-speaker"),
    (dict(sid_decoder_speaker=True), "sid-decoder-speaker"),
    (dict(sid_t5_postnet=True), "sid-t5-postnet"),
    (dict(sid_encoder_cls="encoder"), "sid-encoder-cls"),
    (dict(sid_shuffle_encoder_input=True), "sid-shuffle-encoder-input"),
    (dict(sid_pad_prenet=True), "sid-pad-prenet"),
])
def test_refused_options_raise(fx, over, word):
    with pytest.raises(NotImplementedError, match=word):
        _build(fx, "recipe", **over)


def test_speaker_head_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scratch_scan
    lib = os.path.join(ROOT, "speecht5_amd", "libspeecht5_hip.so")
    ks = [k for k in scratch_scan.kernels(lib) if "margin_" in k[0] or "time_mean" in k[0]]
    assert len(ks) >= 6, ks
    assert all(k[1] == 0 and k[2] == 0 for k in ks), ks
