"""TTS fine-tuning (t2s) on a FIXED-SHAPE batch -- collate.TextToSpeechCollater(fixed_shape=(N, L)) and the live-frame mel post-net
(T5TransformerModel.forward(tgt_live=...), functional.PostnetFunction on st5_batchnorm_act_*_live) -- is the own-length step.  Tiny
fixture model, fp32, every dropout 0 as the fixture has it.

1. The golden sample of tests/golden/tiny_t2s.pt (B 3, 11 text columns, 24 frames) embedded by hand into a (16, 32) batch with
   tgt_live = 12: `before`, `after`, stop logits and alignments on the valid region, the loss terms and check_grads at the tolerances
   tests/test_model_gpu.py::test_t2s_fp32_matches_reference_and_generated_mel uses against the same golden (2e-4; gradients 2e-3).  The
   yardstick is the verbatim reference's recorded output.  The padded region of `after` is exact zeros.
2. The same batch WITHOUT tgt_live: `after` differs from the golden by more than 1e-2 relative (a CPU probe with the oracle measured
   0.95): the post-net's batch statistics and convolutions take the padding in, so test 1 does see the post-net.
3. Four more batches without a golden through both collaters -- frame counts [28, 9, 15], [13, 12, 7], [6, 5, 4], [27, 26, 2], fixed
   shape (12, 28), r = 2, a text row of 12 tokens and one of 1 token among them: loss terms 2e-4, the flat gradient 2e-3, and the
   BatchNorm running statistics after the step 2e-4, fixed shape against own lengths at equal weights.  The measured differences are
   printed, and appended to the file ST5_PARITY_OUT names (how profiles/t2s_fixed_shape_parity.txt was written).
4. The collater: its fixed-shape output equals the own-length collater's output padded by hand, tgt_live is right, plan() refuses
   before anything is launched.
5. Eval mode (running statistics): `after` of a fixed-shape batch against the own-length one."""
import os

import pytest
import torch

from tests.util import Task, build_tiny, check_grads, close, load_golden, to_dev

pytestmark = pytest.mark.gpu
VOCAB = 30
N, L, R = 12, 28, 2
FRAMES = [[28, 9, 15], [13, 12, 7], [6, 5, 4], [27, 26, 2]]
TOKENS = [[12, 5, 7], [1, 9, 4], [3, 3, 3], [12, 1, 6]]


def _report(line):
    print(line)
    path = os.environ.get("ST5_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _model(cuda, train=True):
    model, args = build_tiny(cuda, torch.float32)
    model.use_codebook = False
    assert args.reduction_factor == R
    return (model.train() if train else model.eval()), args


def _crit():
    from speecht5_amd.criterions import TexttoSpeechLoss
    return TexttoSpeechLoss(Task(), False, use_guided_attn_loss=True, guided_attn_loss_sigma=0.4, guided_attn_loss_lambda=10.0,
                            sync_logging=False)


def _reset(model):
    m, _ = load_golden(None)
    torch.nn.Module.load_state_dict(model, m["state_dict"], strict=True)
    for p in model.parameters():
        p.grad = None


def _embed(sample, n_cols, n_frames, live, pad=1):
    """The golden sample padded by hand to (n_cols text columns, n_frames mel frames): pad id, zero frames, labels 1.0 in the tail."""
    s = {k: (dict(v) if isinstance(v, dict) else v) for k, v in sample.items()}
    ni = s["net_input"]
    B, T = ni["src_tokens"].shape
    Lf, odim = s["dec_target"].shape[1:]
    dev = s["dec_target"].device
    tok = torch.full((B, n_cols), pad, dtype=torch.long, device=dev)
    tok[:, :T] = ni["src_tokens"]
    prev = torch.zeros(B, n_frames // R, odim, device=dev)
    prev[:, :ni["prev_output_tokens"].shape[1]] = ni["prev_output_tokens"]
    tgt = torch.zeros(B, n_frames, odim, device=dev)
    tgt[:, :Lf] = s["dec_target"]
    lab = torch.ones(B, n_frames, device=dev)
    lab[:, :Lf] = s["labels"]
    ni.update(src_tokens=tok, prev_output_tokens=prev)
    if live is not None:
        ni["tgt_live"] = torch.tensor([live], dtype=torch.int32, device=dev)
    s.update(dec_target=tgt, labels=lab)
    return s


def _golden_sample(cuda, live):
    _, fx = load_golden("tiny_t2s.pt")
    model, args = _model(cuda)
    return fx, model, _embed(to_dev(fx["sample"], cuda), 16, 32, live)


# ---- 1 ----
def test_golden_sample_in_a_larger_shape_matches_the_reference(cuda):
    fx, model, sample = _golden_sample(cuda, 12)
    loss, _, log = _crit()(model, sample)
    for got, ref, name in ((loss, fx["loss"], "loss"), (log["l1_loss"], fx["l1"], "l1"), (log["bce_loss"], fx["bce"], "bce"),
                           (log["enc_dec_attn_loss"], fx["guided"], "guided attention loss")):
        close(got, ref, 2e-4, what=name)
    loss.backward()
    torch.cuda.synchronize()
    assert check_grads(model, fx, 2e-3) > 40
    _reset(model)
    with torch.no_grad():
        before, after, logits, attn = model(**sample["net_input"])
    assert tuple(before.shape) == tuple(after.shape) == (3, 32, 80) and tuple(logits.shape) == (3, 32)
    for got, ref, name in ((before, fx["out"]["before"], "before"), (after, fx["out"]["after"], "after"),
                           (logits, fx["out"]["stop_logits"], "stop_logits")):
        close(got[:, :24], ref, 2e-4, what=name)
    assert len(attn) == len(fx["out"]["attn"])
    for a, b in zip(attn, fx["out"]["attn"]):
        assert tuple(a.shape) == (3, 2, 16, 16)
        close(a[:, :, :12, :11], b, 2e-4, what="attn")
    assert bool((after[:, 24:] == 0).all()), "`after` behind the live frames"


# ---- 2 ----
def test_without_tgt_live_the_post_net_sees_the_padding(cuda):
    fx, model, sample = _golden_sample(cuda, None)
    with torch.no_grad():
        before, after, logits, attn = model(**sample["net_input"])
    close(before[:, :24], fx["out"]["before"], 2e-4, what="before")          # everything in front of the post-net is masked by lengths
    close(logits[:, :24], fx["out"]["stop_logits"], 2e-4, what="stop_logits")
    ref = fx["out"]["after"].to(cuda)
    rel = float((after[:, :24] - ref).abs().max() / ref.abs().max())
    _report(f"t2s_fixed_shape golden (16, 32) without tgt_live: `after` differs from the reference by {rel:.3e} relative")
    assert rel > 1e-2, rel


# ---- 3 ----
def _items(cuda, k, spk_dim):
    g = torch.Generator().manual_seed(77 + k)
    return [{"id": 10 * k + i, "audio_name": f"u{k}-{i}",
             "source": [torch.cat([torch.randint(4, 4 + VOCAB, (n - 1,), generator=g), torch.tensor([2])]).to(cuda)],
             "target": (torch.randn(f, 80, generator=g) * 0.5 - 1).to(cuda), "spkembs": torch.randn(spk_dim, generator=g).to(cuda)}
            for i, (f, n) in enumerate(zip(FRAMES[k], TOKENS[k]))]


def _step(model, batch):
    _reset(model)
    loss, _, log = _crit()(model, batch)
    loss.backward()
    torch.cuda.synchronize()
    flat = torch.cat([p.grad.reshape(-1) if p.grad is not None else torch.zeros(p.numel(), device=p.device) for p in model.parameters()])
    bn = {n: b.detach().clone() for n, b in model.named_buffers() if "running_" in n or "num_batches_tracked" in n}
    terms = {k: log[k].detach().clone() for k in ("loss", "l1_loss", "l2_loss", "bce_loss", "enc_dec_attn_loss")}
    return terms, flat, bn


_shared = {}


def _both(cuda, k):
    """Batch k through both collaters and one training step each, computed once."""
    if k not in _shared:
        from speecht5_amd.collate import TextToSpeechCollater
        model, args = _model(cuda)
        items = _items(cuda, k, args.spk_embed_dim)
        own = TextToSpeechCollater(cuda, pad_idx=1, reduction_factor=R).collater(items)
        fixed = TextToSpeechCollater(cuda, pad_idx=1, reduction_factor=R, fixed_shape=(N, L)).collater(items)
        _shared[k] = (own, fixed, _step(model, own), _step(model, fixed))
    return _shared[k]


@pytest.mark.parametrize("k", range(len(FRAMES)))
def test_fixed_shape_step_equals_the_own_length_step(cuda, k):
    own, fixed, (t0, g0, bn0), (t1, g1, bn1) = _both(cuda, k)
    assert tuple(fixed["dec_target"].shape) == (3, L, 80) and tuple(own["dec_target"].shape) == (3, max(FRAMES[k]), 80)
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))  # noqa: E731
    _report(f"t2s_fixed_shape batch {FRAMES[k]} x {TOKENS[k]} in ({N}, {L}) against own lengths: "
            + "  ".join(f"{n} {rel(t1[n], t0[n]):.2e}" for n in t0) + f"  flat gradient {rel(g1, g0):.2e}  "
            + f"running statistics {max(rel(bn1[n], bn0[n]) for n in bn0 if 'running_' in n):.2e}")
    for n in t0:
        close(t1[n], t0[n], 2e-4, what=n)
    assert float(g0.abs().max()) > 0 and bool(torch.isfinite(g1).all())
    close(g1, g0, 2e-3, what="flat gradient")
    moved = 0
    m, _ = load_golden(None)
    for n in bn0:
        if "num_batches_tracked" in n:
            assert int(bn1[n]) == int(bn0[n]) == int(m["state_dict"][n]) + 1, n
        else:
            close(bn1[n], bn0[n], 2e-4, what=n)
            moved += int(not torch.equal(bn0[n].cpu(), m["state_dict"][n]))
    assert moved == 10       # (five layers' running mean and variance, all moved by the step)


# ---- 4 ----
@pytest.mark.parametrize("k", range(len(FRAMES)))
def test_fixed_shape_batch_is_the_own_length_batch_padded_further(cuda, k):
    own, fixed = _both(cuda, k)[:2]
    want = _embed(own, N, L, max(FRAMES[k]) // R)
    assert set(fixed) == set(own) and set(fixed["net_input"]) == set(own["net_input"]) | {"tgt_live"}
    ti = fixed["net_input"]["tgt_live"]
    assert ti.dtype == torch.int32 and tuple(ti.shape) == (1,) and ti.is_cuda and int(ti) == max(FRAMES[k]) // R
    for key in ("src_tokens", "src_lengths", "prev_output_tokens", "tgt_lengths", "spkembs"):
        assert torch.equal(fixed["net_input"][key], want["net_input"][key]), key
    for key in ("labels", "dec_target", "dec_target_lengths", "src_lengths", "id", "target"):
        assert torch.equal(fixed[key], want[key] if key != "target" else want["dec_target"]), key
    assert fixed["ntokens"] == own["ntokens"] == sum(TOKENS[k]) and fixed["name"] == own["name"] and fixed["task_name"] == "t2s"
    assert tuple(fixed["net_input"]["src_tokens"].shape) == (3, N) and tuple(fixed["net_input"]["prev_output_tokens"].shape) == (3, L // R, 80)


def test_plan_refuses_before_anything_is_launched(cuda):
    from speecht5_amd.collate import TextToSpeechCollater
    coll = TextToSpeechCollater(cuda, pad_idx=1, reduction_factor=R, fixed_shape=(N, L))
    items = _items(cuda, 0, 64)
    for change, match in (({"target": torch.zeros(29, 80, device=cuda)}, r"item 1: 29 frames"),
                          ({"target": torch.zeros(1, 80, device=cuda)}, r"item 1: 1 frames"),
                          ({"source": [torch.full((13,), 5, device=cuda)]}, r"item 1: 13 tokens")):
        bad = [dict(it) for it in items]
        bad[1].update(change)
        before = torch.cuda.memory_allocated()
        with pytest.raises(ValueError, match=match):
            coll(bad)
        assert torch.cuda.memory_allocated() == before


# ---- 5 ----
def test_eval_mode_after_equals_the_own_length_one(cuda):
    from speecht5_amd.collate import TextToSpeechCollater
    model, args = _model(cuda, train=False)
    items = _items(cuda, 1, args.spk_embed_dim)
    own = TextToSpeechCollater(cuda, pad_idx=1, reduction_factor=R).collater(items)
    fixed = TextToSpeechCollater(cuda, pad_idx=1, reduction_factor=R, fixed_shape=(N, L)).collater(items)
    with torch.no_grad():
        b0, a0, l0, _ = model(**own["net_input"])
        b1, a1, l1, _ = model(**fixed["net_input"])
        no_live = {k: v for k, v in fixed["net_input"].items() if k != "tgt_live"}
        _, a2, _, _ = model(**no_live)
    n = a0.shape[1]
    assert n == 12 and tuple(a1.shape) == (3, L, 80)
    close(b1[:, :n], b0, 2e-4, what="before")
    close(a1[:, :n], a0, 2e-4, what="after")
    close(l1[:, :n], l0, 2e-4, what="stop logits")
    assert bool((a1[:, n:] == 0).all())
    # without the live count the convolutions read the decoder's output at padded steps across the edge
    assert float((a2[:, :n] - a0).abs().max()) > 1e-3 * float(a0.abs().max())
