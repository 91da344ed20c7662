"""st5_ctc_pack_rows, functional.ctc_loss_rows and SpeechtoTextLoss(device_targets=True) on the GPU.
1. the kernel against the numpy restatement (tests/ctc_pack_reference.py), all four outputs `==`: one and several 64-column chunks,
   L on either side of a chunk boundary, more rows than waves, every row kind; garbage-filled outputs (every element is written);
   `total` written, not accumulated, over two launches; the error returns; the launch under stream capture.
2. ctc_loss_rows against ctc_loss_sum on the masked_select form: loss and lprobs.grad the same bits -- a row of target length 0 and
   a zero_infinity case (a target longer than its input) among them.
3. the criterion on the fixture's sample (tests/golden/tiny_s2t.pt): device_targets=True against False -- loss, every parameter
   gradient, every logged entry equal; ntokens equals the host value; with sync_logging=False the forward synchronises nothing
   (torch.cuda.set_sync_debug_mode("error") around the call)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from speecht5_amd import functional as Fn
from speecht5_amd import hip
from tests.ctc_pack_reference import pack_rows, rows_of_every_kind
from tests.util import Task, build_tiny, injected_randomness, load_golden, to_dev

pytestmark = pytest.mark.gpu
PAD, EOS = 1, 2
ST5_ERR_ARG = 1
GARBAGE = -0x0123456789ABCDEF


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _launch(t, packed, offsets, kept, total):
    B, L = t.shape
    return hip.lib().st5_ctc_pack_rows(t.data_ptr(), PAD, EOS, B, L, packed.data_ptr(), offsets.data_ptr(), kept.data_ptr(),
                                       total.data_ptr(), hip.stream())


# ---- 1 ----
@pytest.mark.parametrize("B,L", [(1, 1), (3, 7), (5, 64), (4, 65), (2, 257), (7, 600), (6, 130)])
def test_pack_rows_equals_the_restatement(cuda, B, L):
    host = rows_of_every_kind(B, L, PAD, EOS, 40, seed=B * 1000 + L)
    want = pack_rows(host, PAD, EOS)
    t = torch.from_numpy(host).to(cuda)
    # the binding: fresh outputs
    got = Fn.ctc_pack_rows(t, PAD, EOS)
    for g, w, name in zip(got, want, ("packed", "offsets", "kept", "total")):
        assert g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), w), (name, B, L)
    # the C ABI into garbage-filled buffers: every element of every output is written
    outs = [torch.full(s, GARBAGE, dtype=torch.int64, device=cuda) for s in ((B, L), (B,), (B,), (1,))]
    assert _launch(t, *outs) == 0
    for g, w, name in zip(outs, want, ("packed", "offsets", "kept", "total")):
        assert np.array_equal(g.cpu().numpy(), w), (name, B, L)
    # `total` is written, not accumulated: the same launch again leaves the same value; another batch replaces it
    assert _launch(t, *outs) == 0
    assert int(outs[3].item()) == int(want[3][0])
    other = torch.from_numpy(rows_of_every_kind(B, L, PAD, EOS, 40, seed=77)).to(cuda)
    assert _launch(other, *outs) == 0
    assert int(outs[3].item()) == int(pack_rows(other.cpu().numpy(), PAD, EOS)[3][0])
    assert _same(t, torch.from_numpy(host).to(cuda))      # the input is left alone


def test_pack_rows_error_returns(cuda):
    t = torch.full((3, 7), 5, dtype=torch.int64, device=cuda)
    packed, offsets, kept, total = (torch.full(s, GARBAGE, dtype=torch.int64, device=cuda) for s in ((3, 7), (3,), (3,), (1,)))
    f = hip.lib().st5_ctc_pack_rows
    good = [t.data_ptr(), PAD, EOS, 3, 7, packed.data_ptr(), offsets.data_ptr(), kept.data_ptr(), total.data_ptr(), hip.stream()]
    for i in (0, 5, 6, 7, 8):                                   # a null pointer in every pointer argument
        assert f(*[0 if j == i else a for j, a in enumerate(good)]) == ST5_ERR_ARG, i
    for i, v in ((3, -1), (4, -1), (3, 0), (4, 0)):              # negative sizes; B = 0 and L = 0 are refused, not launched
        assert f(*[v if j == i else a for j, a in enumerate(good)]) == ST5_ERR_ARG, (i, v)
    bad = list(good)
    bad[5] = good[0]                                            # not an in-place operation
    assert f(*bad) == ST5_ERR_ARG
    torch.cuda.synchronize()
    for o in (packed, offsets, kept, total):                    # nothing was launched
        assert bool((o == GARBAGE).all())
    with pytest.raises(ValueError):
        Fn.ctc_pack_rows(t.int(), PAD, EOS)
    with pytest.raises(ValueError):
        Fn.ctc_pack_rows(t[:, :0], PAD, EOS)
    with pytest.raises(ValueError):
        Fn.ctc_pack_rows(t.cpu(), PAD, EOS)


def test_pack_rows_is_capturable_and_replays_on_new_data(cuda):
    B, L = 5, 130
    a = rows_of_every_kind(B, L, PAD, EOS, 40, seed=1)
    b = rows_of_every_kind(B, L, PAD, EOS, 40, seed=2)[::-1].copy()
    t = torch.from_numpy(a).to(cuda)
    outs = [torch.full(s, GARBAGE, dtype=torch.int64, device=cuda) for s in ((B, L), (B,), (B,), (1,))]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        assert _launch(t, *outs) == 0
    for host in (a, b, a):
        t.copy_(torch.from_numpy(host))
        g.replay()
        torch.cuda.synchronize()
        for o, w in zip(outs, pack_rows(host, PAD, EOS)):
            assert np.array_equal(o.cpu().numpy(), w)


# ---- 2 ----
def _ctc_case(cuda, zero_infinity_case):
    """T = 50, B = 3, V = 12, L = 9 columns (label + eos + pad); row 1 has no label at all.  zero_infinity_case: row 2's input is
    shorter than its 8 labels, an impossible alignment."""
    T, B, V, L = 50, 3, 12, 9
    rng = np.random.RandomState(11)
    n = [5, 0, 8]
    target = np.full((B, L), PAD, dtype=np.int64)
    for b, k in enumerate(n):
        target[b, :k] = rng.randint(4, V - 1, size=k)
        target[b, k] = EOS
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(T, B, V, generator=g)
    in_len = torch.tensor([50, 37, 6 if zero_infinity_case else 44])
    return logits.to(cuda), torch.from_numpy(target).to(cuda), in_len.to(cuda), torch.tensor([k + 1 for k in n]).to(cuda), V - 1


@pytest.mark.parametrize("zero_infinity_case", [False, True], ids=["feasible", "zero_infinity"])
def test_ctc_loss_rows_is_bit_equal_to_the_masked_select_form(cuda, zero_infinity_case):
    logits, target, in_len, tgt_len, blank = _ctc_case(cuda, zero_infinity_case)

    def run(rows):
        x = logits.clone().requires_grad_(True)
        lp = torch.log_softmax(x, -1)
        lp.retain_grad()
        if rows:
            loss, total = Fn.ctc_loss_rows(lp, target, in_len, tgt_len - 1, PAD, EOS, blank, True, return_total=True)
        else:
            mask = (target != PAD) & (target != EOS)
            loss = Fn.ctc_loss_sum(lp, target.masked_select(mask), in_len, tgt_len - 1, blank, True, max_target_len=target.size(1))
            total = mask.sum().view(1)
        (loss * 0.37).backward()
        return loss.detach(), lp.grad, x.grad, total
    ref, got = run(False), run(True)
    assert torch.isfinite(ref[0]) and float(ref[0]) > 0
    for r, g, name in zip(ref, got, ("loss", "lprobs.grad", "logits.grad", "total")):
        assert _same(r, g), (name, r, g)
    assert int(got[3]) == 13
    if zero_infinity_case:      # the impossible row contributes nothing: no loss, no gradient
        assert not bool(got[1][:, 2].any()) and bool(got[1][:, 0].any())
    # without the return_total keyword the issue's signature returns the loss alone
    lp = torch.log_softmax(logits, -1)
    assert _same(Fn.ctc_loss_rows(lp, target, in_len, tgt_len - 1, PAD, EOS, blank, True), got[0])


# ---- 3 ----
LABELS = 14      # the fixture's labels: 8 + 6; its target_lengths (label + </s>) are 9 and 7


def _criterion_run(cuda, device_targets, sync_logging, guard=False, verbatim=False):
    """The fixture's sample carries ntokens = 16 = target_lengths.sum(), </s> counted (oracle/make_golden.py wrote it by hand).  The
    collaters -- the reference's collater_seq_label and collate.SpeechToTextCollater -- count the labels alone, and that is what the
    pack kernel counts.  Unless `verbatim`, the sample therefore carries the collater's ntokens (14); everything else is the fixture's."""
    from speecht5_amd.criterions import SpeechtoTextLoss
    _, fx = load_golden("tiny_s2t.pt")
    model, _ = build_tiny(cuda, torch.float32)
    model.speech_encoder_prenet.mask_prob = 0.5
    model.train()
    sample = to_dev(fx["sample"], cuda)
    assert int((fx["sample"]["target_lengths"] - 1).sum()) == LABELS and fx["sample"]["ntokens"] == LABELS + 2
    if not verbatim:
        sample["ntokens"] = LABELS
    # (what the collater attaches: the padding mask's host copy, so that the span-mask draw reads nothing from the device)
    sample["net_input"]["padding_mask"]._st5_host = fx["sample"]["net_input"]["padding_mask"].clone()
    crit = SpeechtoTextLoss(SimpleNamespace(zero_infinity=True), Task(), sentence_avg=False, label_smoothing=0.1, report_accuracy=True,
                            ce_weight=0.5, ctc_weight=0.5, sync_logging=sync_logging, device_targets=device_targets)
    try:
        Fn.manual_seed(3)
        # (the recorded Gumbel noise is moved to the device here: the injection's own `.to(device)` inside the forward would be a
        #  synchronising copy of the test's, not of the product's)
        with injected_randomness(model, fx["mask_indices"], fx["mix_idx"], fx["gumbel_noise"].to(cuda), fx["tau"]):
            if guard:
                crit(model, sample)      # (first call: weight caches, workspaces)
                Fn.manual_seed(3)
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
            try:
                loss, sample_size, log = crit(model, sample)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        (loss / sample_size).backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        return loss.detach().clone(), sample_size, log, grads, fx
    finally:
        Fn.weight_cache.clear()
        Fn.bf16_mirror.__init__()


_ref = {}


def _reference(cuda):
    """The masked_select mode with host logging, run once, shared, never modified."""
    if "run" not in _ref:
        _ref["run"] = _criterion_run(cuda, False, True)
    return _ref["run"]


def test_criterion_device_targets_equals_the_masked_select_mode(cuda):
    ref_loss, ref_ss, ref_log, ref_grads, fx = _reference(cuda)
    loss, ss, log, grads, _ = _criterion_run(cuda, True, True)
    assert _same(ref_loss, loss) and ss == ref_ss == LABELS
    assert sorted(grads) == sorted(ref_grads) and len(grads) > 40
    for n in grads:
        assert _same(ref_grads[n], grads[n]), n
    assert list(log) == list(ref_log)
    for k in log:
        assert log[k] == ref_log[k] and type(log[k]) is type(ref_log[k]), (k, log[k], ref_log[k])
    assert log["ntokens"] == LABELS and float(log["ctc_loss"]) > 0


def test_criterion_on_the_verbatim_fixture_sample(cuda):
    """The fixture's own ntokens (16, </s> counted) is not the collater's: loss (sample_size is the host value in both modes),
    gradients and every other entry are equal; the logged ntokens is the kernel's count of labels, 14."""
    ref_loss, ref_ss, ref_log, ref_grads, fx = _criterion_run(cuda, False, True, verbatim=True)
    loss, ss, log, grads, _ = _criterion_run(cuda, True, True, verbatim=True)
    assert _same(ref_loss, loss) and ss == ref_ss == fx["sample_size"] == LABELS + 2
    for n in grads:
        assert _same(ref_grads[n], grads[n]), n
    for k in log:
        assert k == "ntokens" or log[k] == ref_log[k], (k, log[k], ref_log[k])
    assert ref_log["ntokens"] == LABELS + 2 and log["ntokens"] == LABELS


def test_criterion_device_targets_forward_reads_nothing_from_the_device(cuda):
    ref_loss, _, ref_log, ref_grads, fx = _reference(cuda)
    loss, ss, log, grads, _ = _criterion_run(cuda, True, False, guard=True)
    assert _same(ref_loss, loss)
    for n in grads:
        assert _same(ref_grads[n], grads[n]), n
    nt = log["ntokens"]
    assert torch.is_tensor(nt) and nt.is_cuda and nt.dtype == torch.int64 and nt.dim() == 0 and int(nt) == LABELS
    for k, v in log.items():
        assert (float(v) if torch.is_tensor(v) else v) == ref_log[k], (k, v, ref_log[k])
    assert ss == LABELS      # (sentence_avg=False: the host value, as without the keyword)
