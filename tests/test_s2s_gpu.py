"""Speech-to-speech fine-tuning (t5_task s2s: voice conversion, speech enhancement through --se-predict / --se-decoder-input) on the
HIP path against the verbatim reference (tests/golden/tiny_s2s.pt, tools/make_golden_s2s.py): the collater bit for bit, the
se_predict kernels against fp64, whole-model / criterion / gradient parity per case, generate_speech from a speech source, and the
ragged log-mel (LogMelFilterBank.rows) against the oracle.  Measured figures: profiles/s2s_parity.txt (tools/s2s_parity.py)."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import logmel_oracle as O
from tests.util import G, close, to_dev

pytestmark = pytest.mark.gpu

CASES = ["recipe", "source_in", "masking", "target", "delta", "delta_prev"]
SETS = ["one", "equal", "odd_target", "one_frame", "single_frame", "longest_first"]
# (the issue's shapes -- every one a whole number of 16-byte vectors or all tail -- plus one with a vector body AND a tail)
SE_SHAPES = [(2, 7, 80), (3, 33, 20), (1, 1, 3), (3, 5, 7)]
ROW_LENGTHS = [513, 1024, 2560, 3333]


@pytest.fixture(scope="module")
def fx():
    return torch.load(os.path.join(G, "tiny_s2s.pt"), weights_only=False)


class S2sTask:
    def __init__(self):
        from tests.util import Dictionary
        self.dicts = {"text": Dictionary(30, ["<mask>", "<ctc_blank>"])}
        self.t5_task = "s2s"
        self.target_dictionary = self.dicts["text"]
        self.blank_symbol_idx = self.dicts["text"].index("<ctc_blank>")


# ---- collater --------------------------------------------------------------------------------------------------------------------
def _same_batch(got, ref, what):
    assert set(got) == set(ref) and set(got["net_input"]) == set(ref["net_input"]), what
    for where, g, r in (("", got, ref), ("net_input.", got["net_input"], ref["net_input"])):
        for k, v in r.items():
            if torch.is_tensor(v):
                a = g[k].cpu()
                assert a.dtype == v.dtype and a.shape == v.shape and torch.equal(a, v), (what, where + k)
            elif k != "net_input":
                assert g[k] == v and type(g[k]) is type(v), (what, where + k)
    assert got["target"] is got["dec_target"]


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("name", SETS)
def test_collater_bit_identical_to_reference(cuda, fx, name, r):
    from speecht5_amd.collate import SpeechToSpeechCollater
    col = fx["collate"][name]
    got = SpeechToSpeechCollater(cuda, reduction_factor=r)(to_dev(col["items"], cuda))
    torch.cuda.synchronize()
    _same_batch(got, col["batches"][r], f"{name} r={r}")
    assert got["net_input"]["source"].is_cuda and not got["src_lengths"].is_cuda and not got["id"].is_cuda


class SpeechToSpeechDataset:
    """Stands in for the reference dataset class (same name, same attributes the wrapper reads)."""

    def __init__(self, items, r):
        self.items, self.reduction_factor, self.tgt_audios = items, r, [it["tgt_name"] for it in items]

    def __getitem__(self, i):
        return self.items[i]

    def __len__(self):
        return len(self.items)

    def ordered_indices(self):
        return list(range(len(self.items)))


def test_wrapped_dataset_collates_on_the_gpu(cuda, fx):
    from speecht5_amd.collate import SpeechToSpeechCollater
    from speecht5_amd.data import GpuCollated, wrap_datasets
    col = fx["collate"]["odd_target"]
    ds = wrap_datasets(SpeechToSpeechDataset(col["items"], 2), cuda)
    assert isinstance(ds, GpuCollated) and isinstance(ds.gpu_collater, SpeechToSpeechCollater) and ds.gpu_collater.reduction_factor == 2
    assert len(ds) == 3 and ds.ordered_indices() == [0, 1, 2] and ds[0]["source"].is_cuda and ds[0]["target"].is_cuda
    _same_batch(ds.collater([ds[i] for i in range(3)]), col["batches"][2], "wrapped s2s")
    assert ds.collater([]) == {}


def test_collater_computes_missing_targets_in_one_ragged_pass(cuda):
    """Items without "target" get the log-mel of their "target_wav" from LogMelFilterBank.rows (one pass for all of them); the batch
    equals the one collated from those frames given as "target"."""
    from speecht5_amd.collate import SpeechToSpeechCollater
    from speecht5_amd.features import LogMelFilterBank
    g = torch.Generator().manual_seed(4)
    wavs = [(torch.randn(n, generator=g) * 0.1).to(cuda) for n in (1500, 700, 2600)]
    fb = LogMelFilterBank(cuda)
    packed, off = fb.rows([wavs[0], wavs[2]])
    given = torch.randn(4, 80, generator=g).to(cuda)
    base = [dict(id=i, source=(torch.randn(300 + 50 * i, generator=g)).to(cuda), spkembs=torch.randn(8, generator=g).to(cuda),
                 audio_name=f"a{i}", tgt_name=f"t{i}") for i in range(3)]
    lazy = [dict(base[0], target=None, target_wav=wavs[0]), dict(base[1], target=given), dict(base[2], target=None, target_wav=wavs[2])]
    eager = [dict(base[0], target=packed[off[0]:off[1]]), dict(base[1], target=given), dict(base[2], target=packed[off[1]:off[2]])]
    col = SpeechToSpeechCollater(cuda, reduction_factor=2, logmel=fb)
    a, b = col(lazy), col(eager)
    torch.cuda.synchronize()
    assert a["dec_target"].shape == (3, 1 + 2600 // 256, 80) and a["dec_target_lengths"].tolist() == [1 + 1500 // 256, 4, 1 + 2600 // 256]
    for k in ("dec_target", "labels", "dec_target_lengths"):
        assert torch.equal(a[k], b[k]), k
    for k in ("prev_output_tokens", "tgt_lengths", "source", "padding_mask"):
        assert torch.equal(a["net_input"][k], b["net_input"][k]), k
    with pytest.raises(ValueError, match="target_wav"):
        col([dict(base[0], target=None)])


# ---- se_predict kernels against fp64 --------------------------------------------------------------------------------------------------
def se_inputs(shape, seed):
    """x of both post-net outputs with |x| up to 30 (s (1 - s) underflows there), src with exact zeros, upstream gradients."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    before, after = torch.randn(shape, generator=g) * 3, torch.randn(shape, generator=g) * 3
    edge = torch.tensor([30.0, -30.0, 20.0, -20.0, 0.0, 12.5, -12.5, 88.0, -88.0])
    before.view(-1)[:min(n, 9)] = edge[:min(n, 9)]
    after.view(-1)[-min(n, 9):] = edge[:min(n, 9)]
    src = torch.randn(shape, generator=g) * 2
    src.view(-1)[::5] = 0.0
    return before, after, src, torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def se_restatement(before, after, src, db, da, mode):
    """speecht5.py:941-949 in torch, in the dtype / on the device of its inputs: outputs and the gradients autograd gives for them."""
    before, after = before.clone().requires_grad_(True), after.clone().requires_grad_(True)
    if mode == "masking":
        yb, ya = torch.sigmoid(before) * src, torch.sigmoid(after) * src
    else:
        yb, ya = before - src, after - src
    torch.autograd.backward([yb, ya], [db, da])
    return yb.detach(), ya.detach(), before.grad, after.grad


def se_errors(cuda, shape, mode, seed=0):
    """Max abs error against the fp64 restatement of (forward, backward) for torch's own fp32 run on the device and for the kernels."""
    from speecht5_amd import functional as Fn
    ins = se_inputs(shape, seed)
    ref = se_restatement(*[t.double() for t in ins], mode)
    t32 = se_restatement(*[t.to(cuda) for t in ins], mode)
    before, after, src, db, da = [t.to(cuda) for t in ins]
    before.requires_grad_(True), after.requires_grad_(True), src.requires_grad_(True)
    yb, ya = Fn.se_predict(before, after, src, Fn.SE_MASKING if mode == "masking" else Fn.SE_DELTA)
    torch.autograd.backward([yb, ya], [db, da])
    torch.cuda.synchronize()
    assert src.grad is None                                   # src_tokens is data
    ours = (yb.detach(), ya.detach(), before.grad, after.grad)
    assert all(torch.isfinite(t).all() for t in ours)

    def err(ts, sl):
        return max((a.double().cpu() - b).abs().max().item() for a, b in zip(ts[sl], ref[sl]))
    f, b = slice(0, 2), slice(2, 4)
    return dict(torch_fwd=err(t32, f), ours_fwd=err(ours, f), torch_bwd=err(t32, b), ours_bwd=err(ours, b)), ours, ins


@pytest.mark.parametrize("mode", ["masking", "delta"])
@pytest.mark.parametrize("shape", SE_SHAPES)
def test_se_predict_kernels_match_fp64(cuda, shape, mode):
    """Bar: twice the error of torch's own fp32 evaluation on the device against fp64, for the same inputs (profiles/s2s_parity.txt
    holds both figures per shape)."""
    e, ours, ins = se_errors(cuda, shape, mode)
    print(f"se_predict {mode} {shape}: {e}")
    assert e["ours_fwd"] <= 2 * e["torch_fwd"], e
    assert e["ours_bwd"] <= 2 * e["torch_bwd"], e
    before, after, src = ins[:3]
    z = src.eq(0)
    if mode == "masking":                                    # src = 0 silences the output and the gradient, exactly
        assert (ours[0].cpu()[z] == 0).all() and (ours[2].cpu()[z] == 0).all()
        big = before.abs() >= 20.0                           # the tails: no NaN from 0 * inf, the gradient dies out
        assert (ours[2].cpu()[big].abs() <= 1e-6).all()


def test_se_predict_scalar_path_for_unaligned_pointers(cuda):
    """Views that start 4 bytes into a buffer: no 16-byte vectors, same values as the aligned call."""
    from speecht5_amd import hip
    g = torch.Generator().manual_seed(9)
    n = 1003
    bufs = [(torch.randn(n + 1, generator=g) * 3).to(cuda) for _ in range(3)]
    outs = [torch.full((n + 1,), float("nan"), device=cuda) for _ in range(4)]
    L = hip.lib()
    for mode in (0, 1):
        a = [b[1:] for b in bufs]                           # unaligned views
        c = [b[1:].clone() for b in bufs]                   # aligned copies
        hip.check(L.st5_se_predict_fwd(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), outs[0][1:].data_ptr(), outs[1][1:].data_ptr(),
                                       n, mode, hip.stream()), "fwd")
        hip.check(L.st5_se_predict_fwd(c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                       n, mode, hip.stream()), "fwd")
        torch.cuda.synchronize()
        assert torch.equal(outs[0][1:], outs[2][:n]) and torch.equal(outs[1][1:], outs[3][:n])
        assert torch.isnan(outs[0][0]) and torch.isnan(outs[2][n])            # nothing written outside [0, n)
    assert L.st5_se_predict_fwd(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), n, 2,
                                hip.stream()) == 1                            # unknown mode: bad argument


# ---- model and criterion against the fixture ----------------------------------------------------------------------------------------
def build_case(fx, name, dev, **over):
    from speecht5_amd import functional as Fn
    from speecht5_amd.speecht5 import T5TransformerModel
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()
    case = fx["cases"][name]
    r = case["case"]["r"]
    model = T5TransformerModel.build_model(Namespace(**dict(case["args"], **over)), S2sTask())
    tiny = torch.load(os.path.join(G, "tiny_model.pt"), weights_only=False)["state_dict"]
    sd = {k: tiny[k] for k in fx["trunk_keys"][r]}
    sd.update(fx["state"][r])
    torch.nn.Module.load_state_dict(model, {k: sd[k] for k in model.state_dict()}, strict=True)
    return model.to(dev)


def case_sample(fx, name, dev):
    case = fx["cases"][name]
    s = to_dev(fx["samples"][case["case"]["r"]], dev)
    s["net_input"] = dict(s["net_input"], **to_dev(case["net_input_extra"], dev))
    s["target"] = s["dec_target"]
    return s


def case_errors(fx, name, dev):
    """Runs one case the way the fixture was recorded and returns (model, what was computed)."""
    from speecht5_amd.criterions import SpeechT5Criterion
    case = fx["cases"][name]
    model = build_case(fx, name, dev)
    sample = case_sample(fx, name, dev)
    model.train()
    out = model(**sample["net_input"])
    model = build_case(fx, name, dev)                       # (the forward above moved the BatchNorm running statistics)
    model.train()
    crit = SpeechT5Criterion(S2sTask(), use_guided_attn_loss=bool(case["case"].get("guided")))
    loss, ss, log = crit(model, sample)
    (loss / ss).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    return model, sample, out, loss, ss, log, grads


@pytest.mark.parametrize("name", CASES)
def test_tiny_fp32_matches_reference(cuda, fx, name):
    """Tolerances: outputs and loss terms 2e-4 of the tensor's scale (tests/test_model_gpu.py test_t2s_fp32_..., tests/test_criterions_gpu.py
    test_t2s_criterion), logged floats 3e-4 (test_criterions_gpu.py), gradient norms 2e-3 of their own size + 1e-4 of the step's largest
    norm and full gradients 2e-3 with that floor (tests/test_sid_gpu.py test_tiny_fp32_matches_reference)."""
    from speecht5_amd import fairseq_compat as fc
    from speecht5_amd.criterions import SpeechT5Criterion
    case = fx["cases"][name]
    model, sample, out, loss, ss, log, got = case_errors(fx, name, cuda)
    before, after, logits, attn = out
    for g, k in ((before, "before"), (after, "after"), (logits, "stop_logits")):
        close(g, case["train"][k], 2e-4, what=f"{name} train {k}")
    assert len(attn) == len(case["train"]["attn"])
    for a, b in zip(attn, case["train"]["attn"]):
        close(a, b, 2e-4, what=f"{name} attn")
    close(loss, case["loss"], 2e-4, what=f"{name} loss")
    assert ss == case["sample_size"] == 1
    assert set(log) == set(case["log"]), (sorted(log), sorted(case["log"]))
    for k, v in case["log"].items():
        assert abs(log[k] - v) <= 3e-4 * max(abs(v), 1.0), (k, log[k], v)
    assert type(log["ntokens"]) is int and log["nsentences"] == 3
    # reduce_metrics: the verbatim function's calls for this logging output
    fc.metrics.reset()
    SpeechT5Criterion.reduce_metrics([{"loss": float(loss.detach()) / ss, "sample_size": 1, "ntokens": log["ntokens"], "s2s": log}])
    calls = [list(c) for c in fc.metrics.recorded]
    assert [c[:2] for c in calls] == [c[:2] for c in case["reduce_calls"]]
    for c, rc in zip(calls, case["reduce_calls"]):
        assert abs(c[2] - rc[2]) <= 3e-4 * max(abs(rc[2]), 1.0) and c[3:] == rc[3:], (c, rc)
    # gradients
    scale = max(case["grads"]["norms"].values())
    for n, ref in case["grads"]["norms"].items():
        g = float(got[n].double().norm()) if n in got else 0.0
        assert abs(g - ref) <= 2e-3 * ref + 1e-4 * scale, (n, g, ref)
    for n, ref in case["grads"]["full"].items():
        close(got[n], ref, 2e-3, what=f"{name} grad {n}", floor=1e-4 * scale)
    # eval mode
    model = build_case(fx, name, cuda)
    model.eval()
    with torch.no_grad():
        _, after, logits, _ = model(**sample["net_input"])
    close(after, case["eval"]["after"], 2e-4, what=f"{name} eval after")
    close(logits, case["eval"]["stop_logits"], 2e-4, what=f"{name} eval stop_logits")


@pytest.mark.parametrize("name", ["recipe", "masking"])
def test_generate_speech_from_a_speech_source(cuda, fx, name):
    """generate_speech(source=..., padding_mask=...) of one clip against the reference's mel / stop probabilities; the bar of the tiny
    t2s synthesis test (tests/test_model_gpu.py: 1e-3 relative)."""
    case = fx["cases"][name]
    model = build_case(fx, name, cuda)
    model.eval()
    wav = fx["gen_clip"].to(cuda)
    spk = fx["samples"][case["case"]["r"]]["net_input"]["spkembs"][:1].to(cuda)
    mel, probs, attn = model.generate_speech(source=wav, padding_mask=torch.zeros(wav.shape, dtype=torch.bool, device=cuda), spkembs=spk)
    close(mel, case["generated_mel"], 1e-3, what="generated mel (TTS parity bar: 1e-3 relative)")
    close(probs, case["generated_probs"], 1e-3, what="stop probabilities")


# ---- refusals and invariants ---------------------------------------------------------------------------------------------------------
def test_se_predict_with_reduction_factor_two_raises(cuda, fx):
    model = build_case(fx, "source_in", cuda, se_predict="masking")
    model.train()
    with pytest.raises(AssertionError, match="2 != 1"):
        model(**case_sample(fx, "source_in", cuda)["net_input"])


def test_unknown_se_predict_raises(cuda, fx):
    model = build_case(fx, "masking", cuda, se_predict="mask")
    model.train()
    with pytest.raises(ValueError, match=r"mask not in \[masking, target, delta\]"):
        model(**case_sample(fx, "masking", cuda)["net_input"])


@pytest.mark.parametrize("shape", [(3, 8, 80), (2, 9, 80), (3, 9, 40), (3, 9, 80, 1), (4, 3, 9, 80)])
def test_src_tokens_the_broadcast_rejects_raise(cuda, fx, shape):
    """The decoder output is [3, 9, 80]: a src_tokens that torch's `sigmoid(out) * src_tokens` would refuse -- or that would enlarge
    the output -- raises before a kernel sees it."""
    model = build_case(fx, "delta_prev", cuda)
    model.train()
    ni = dict(case_sample(fx, "delta_prev", cuda)["net_input"], src_tokens=torch.zeros(shape, device=cuda))
    with pytest.raises(RuntimeError):
        model(**ni)
    with pytest.raises(TypeError):
        model(**dict(ni, src_tokens=None))


def test_broadcastable_src_tokens_runs_as_the_reference_expression(cuda, fx):
    model = build_case(fx, "delta_prev", cuda)
    model.eval()
    ni = case_sample(fx, "delta_prev", cuda)["net_input"]
    row = ni["src_tokens"][:1, :1].contiguous()             # [1, 1, 80] broadcasts over batch and time
    with torch.no_grad():
        a = model(**dict(ni, src_tokens=row))[1]
        b = model(**dict(ni, src_tokens=row.expand(3, 9, 80).contiguous()))[1]
    assert torch.equal(a, b)


def test_without_se_predict_the_route_is_the_existing_one(cuda, fx):
    """The recipe case carries no se_predict: its outputs are the fixture's (asserted per case above) and setting the option to None
    explicitly -- what the command line gives when the flag is absent from a namespace that declares it -- changes nothing, bit for bit."""
    case = fx["cases"]["recipe"]
    assert "se_predict" not in case["args"]
    sample = case_sample(fx, "recipe", cuda)
    outs = []
    for over in ({}, {"se_predict": None}):
        model = build_case(fx, "recipe", cuda, **over)
        model.train()
        outs.append(model(**sample["net_input"]))
    close(outs[0][1], case["train"]["after"], 2e-4, what="recipe after")
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)


def test_prune_modules_keeps_the_reference_key_list(cuda, fx):
    model = build_case(fx, "recipe", torch.device("cpu"))
    model.prune_modules("s2s")
    assert list(model.state_dict().keys()) == fx["pruned_keys"]


# ---- ragged log-mel -----------------------------------------------------------------------------------------------------------------
def rows_case(cuda):
    """LogMelFilterBank.rows over the four lengths in one call: 513 = the minimum legal length, 1024 = exactly one FFT, 2560 = a
    multiple of the hop, 3333 = a ragged tail.  Returns (waveforms, per-item outputs of rows, per-item outputs of __call__)."""
    from speecht5_amd.features import LogMelFilterBank
    fb = LogMelFilterBank(cuda)
    g = torch.Generator().manual_seed(13)
    wavs = [torch.randn(n, generator=g) * 0.1 for n in ROW_LENGTHS]
    packed, off = fb.rows([w.to(cuda) for w in wavs])
    torch.cuda.synchronize()
    assert off == [0] + list(np.cumsum([1 + n // 256 for n in ROW_LENGTHS])) and packed.shape == (off[-1], 80)
    rows = [packed[off[i]:off[i + 1]].cpu() for i in range(len(wavs))]
    single = [fb(w[None].to(cuda))[0].cpu() for w in wavs]
    return fb, wavs, rows, single


def test_ragged_logmel_matches_oracle(cuda):
    fb, wavs, rows, single = rows_case(cuda)
    for w, got, one in zip(wavs, rows, single):
        orc = O.logmelfilterbank(w.numpy())
        assert got.shape == orc.shape
        # the bar of tests/test_logmel.py: fp32 DFT of 1024 points seen through log10 near the floor
        assert np.abs(got.numpy() - orc).max() < 2e-3, (len(w), np.abs(got.numpy() - orc).max())
        # the item alone through __call__: measured difference 0 at every length (profiles/s2s_parity.txt), so it is held to that
        assert torch.equal(got, one), (len(w), (got - one).abs().max().item())
    with pytest.raises(ValueError, match="reflect padding needs more than 512 samples, got 512"):
        fb.rows([wavs[1].to(cuda), torch.zeros(512, device=cuda)])
