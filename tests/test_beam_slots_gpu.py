"""Beam search over a slot cache with sentence-shared cross-attention (SequenceGenerator(decode="slots"),
TransformerDecoder.init_beam_slots, csrc/beam_decode.hip).

1. st5_beam_cross_attn against the fp64 restatement of tests/beam_slots_reference.py at the tolerances tests/test_tts_batch_gpu.py
   holds st5_decode_cross_attn to (1e-5 fp32, 2e-2 bf16, of the tensor scale): beams 1 ... 17, S in one workgroup and split, fewer live
   sentences than stored ones with a permuted `sent`, fully padded tails, K|V at a column offset of wider rows, the probability record
   on and off (ctx bit-equal), more heads than one workgroup takes, head_dim 80 refused, a bad `sent` entry;
2. bit-identity: a sentence alone = among 7 others, permuted rows = permuted bits, duplicate queries = duplicate bits;
3. the tiny model: every case of tests/golden/tiny_s2t_beam.pt and tiny_s2t_beam_lm.pt decoded with decode="slots" returns the
   reference generator's hypotheses; ctc_rows / exact_rows with slots against the same options with concat;
4. Base size and the pre-LN tiny-Large configuration: the slot state driven along the trajectory recorded from a `concat` run, every
   step's log-probabilities compared (fp32: the 2e-3 positional bar of tests/test_generator_gpu.py; bf16: against the fp32 concat
   run, at most BF16_MARGIN x the concat bf16 path's own worst error);
5. no copies: the K/V buffers and the encoder rows stay where they are through a generate(), reorder_encoder_out is never called.
Figures go to the file ST5_PARITY_OUT names (how profiles/beam_slots_parity.txt was written)."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.beam_slots_reference import SlotSim, beam_cross_attn_ref, synthetic_sequence
from tests.test_generator_gpu import SCORE_TOL
from tests.util import Task, build_tiny, close, load_golden, to_dev

pytestmark = pytest.mark.gpu

POS_TOL = 2e-3        # the positional-score bar of tests/test_generator_gpu.py / test_lm_fusion_gpu.py
BF16_MARGIN = 2.0     # slot path's worst bf16 error <= this x the concat path's on the same trajectory (different summation order)


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


def _report(line):
    print(line)
    path = os.environ.get("ST5_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the fp64 restatement
# ------------------------------------------------------------------------------------------------------------------------------
def _kernel_case(seed, dtype, n_sent, n_live, beam, S, H, k_off=16, extra=24):
    g = torch.Generator().manual_seed(seed)
    C = H * 64
    ld = k_off + 2 * C + extra
    kv = (torch.randn(n_sent * S, ld, generator=g) * 2).to(dtype)
    q = torch.randn(n_live * beam, C, generator=g).to(dtype)
    sent = torch.randperm(n_sent, generator=g)[:n_live].to(torch.int32)
    lens = torch.randint(1, S + 1, (n_sent,), generator=g)
    lens[int(sent[0])] = S                               # one sentence without padding
    if n_live > 1:
        lens[int(sent[1])] = max(1, S // 3)              # a fully padded tail: whole key ranges of the split path hold no valid key
    kpm = (torch.arange(S)[None, :] >= lens[:, None]).to(torch.uint8)
    return q, kv, k_off, sent, kpm


def _run_kernel(cuda, q, kv, k_off, sent, kpm, n_sent, beam, S, H, record=True):
    from speecht5_amd import functional as Fn
    rows = q.shape[0]
    rec = None
    probs = None
    if record:
        rec = torch.full((rows, H, 3, S), 7.0, device=cuda)          # the step's column inside a larger record
        probs = (rec[:, :, 1], rec.stride(0), rec.stride(1))
    ctx = Fn.beam_cross_attn(q.to(cuda), kv.to(cuda), k_off, sent.to(cuda), n_sent, beam, S, H, 64,
                             kpm=None if kpm is None else kpm.to(cuda), probs=probs)
    torch.cuda.synchronize()
    return ctx, rec


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S", [7, 64, 65, 499, 1500])
@pytest.mark.parametrize("beam", [1, 3, 4, 10, 16, 17])
def test_kernel_matches_fp64(cuda, beam, S, dtype):
    H = 12 if S == 499 else 4
    n_sent, n_live = 5, 3
    q, kv, k_off, sent, kpm = _kernel_case(100 * beam + S, dtype, n_sent, n_live, beam, S, H)
    ctx, rec = _run_kernel(cuda, q, kv, k_off, sent, kpm, n_sent, beam, S, H)
    ctx2, _ = _run_kernel(cuda, q, kv, k_off, sent, kpm, n_sent, beam, S, H, record=False)
    ref_ctx, ref_p = beam_cross_attn_ref(q, kv, k_off, sent.tolist(), n_sent, beam, S, H, kpm=kpm)   # (sees the rounded inputs)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    close(ctx, ref_ctx, tol, what=f"ctx beam={beam} S={S}")
    assert torch.equal(ctx, ctx2), "ctx depends on the probability write"
    p = rec[:, :, 1].cpu()
    close(p, ref_p, tol, what="probabilities")
    masked = kpm.bool()[sent.long().repeat_interleave(beam)][:, None, :].expand(n_live * beam, H, S)
    assert (p[masked] == 0).all(), "an excluded key must get probability exactly 0"
    assert (p.double().sum(-1) - 1).abs().max() < 1e-4
    assert (rec[:, :, 0] == 7.0).all() and (rec[:, :, 2] == 7.0).all(), "record columns other than the step's were written"


@pytest.mark.parametrize("H,beam,S", [(12, 10, 70), (16, 16, 33), (20, 10, 70), (33, 5, 9), (64, 3, 80)])
def test_kernel_head_counts(cuda, H, beam, S):
    """More heads than fit one query image at 16 rows (H 20: 8 rows per workgroup) and more than one workgroup takes (H > 32)."""
    n_sent, n_live = 3, 2
    q, kv, k_off, sent, kpm = _kernel_case(7 * H + S, torch.float32, n_sent, n_live, beam, S, H, k_off=0, extra=0)
    ctx, rec = _run_kernel(cuda, q, kv, k_off, sent, kpm, n_sent, beam, S, H)
    ref_ctx, ref_p = beam_cross_attn_ref(q, kv, k_off, sent.tolist(), n_sent, beam, S, H, kpm=kpm)
    close(ctx, ref_ctx, 1e-5, what=f"ctx H={H}")
    close(rec[:, :, 1], ref_p, 1e-5, what=f"probabilities H={H}")


def test_kernel_without_padding_mask(cuda):
    q, kv, k_off, sent, _ = _kernel_case(5, torch.float32, 4, 4, 3, 100, 4)
    ctx, rec = _run_kernel(cuda, q, kv, k_off, sent, None, 4, 3, 100, 4)
    ref_ctx, ref_p = beam_cross_attn_ref(q, kv, k_off, sent.tolist(), 4, 3, 100, 4)
    close(ctx, ref_ctx, 1e-5, what="ctx")
    close(rec[:, :, 1], ref_p, 1e-5, what="probabilities")


def test_head_dim_80_is_rejected_and_alignment_is_checked(cuda):
    from speecht5_amd import hip
    L = hip.lib()
    q = torch.zeros(4, 160, device=cuda)
    kv = torch.zeros(8, 320, device=cuda)
    sent = torch.zeros(2, dtype=torch.int32, device=cuda)
    ctx = torch.zeros(4, 160, device=cuda)

    def call(hd=64, H=2, kv_ld=320, k_off=0, qp=None):
        return L.st5_beam_cross_attn(qp or q.data_ptr(), 160, kv.data_ptr(), kv_ld, k_off, 0, sent.data_ptr(), 2, 2, 2, 4, H, hd,
                                     ctx.data_ptr(), 160, 0, 0, 0, 0, hip.F32, hip.stream())
    assert call(hd=80) == 1, "head_dim 80 must be ST5_ERR_ARG"
    assert call(H=65) == 1
    assert call(kv_ld=322) == 2 and call(k_off=2, kv_ld=324) == 2 and call(qp=q.data_ptr() + 4) == 2, "ST5_ERR_ALIGN"
    assert call() == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("S", [20, 200])
@pytest.mark.parametrize("bad", [-1, 5])
def test_bad_sent_entry_gives_nan_in_that_sentence_only(cuda, S, bad):
    n_sent, n_live, beam, H = 5, 3, 4, 4
    q, kv, k_off, sent, kpm = _kernel_case(31 + S, torch.float32, n_sent, n_live, beam, S, H)
    good, good_rec = _run_kernel(cuda, q, kv, k_off, sent, kpm, n_sent, beam, S, H)
    sent_bad = sent.clone()
    sent_bad[1] = bad
    ctx, rec = _run_kernel(cuda, q, kv, k_off, sent_bad, kpm, n_sent, beam, S, H)
    assert torch.isnan(ctx[beam:2 * beam]).all() and torch.isnan(rec[beam:2 * beam, :, 1]).all()
    keep = torch.cat([torch.arange(0, beam), torch.arange(2 * beam, 3 * beam)]).to(cuda)
    assert torch.equal(ctx[keep], good[keep]) and torch.equal(rec[keep], good_rec[keep])


# ------------------------------------------------------------------------------------------------------------------------------
# 2. bit-identity
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S", [40, 499])
def test_bits_do_not_depend_on_the_launch(cuda, S, dtype):
    from speecht5_amd import functional as Fn
    n_sent, beam, H = 8, 10, 12
    q, kv, k_off, sent, kpm = _kernel_case(77 + S, dtype, n_sent, n_sent, beam, S, H)
    qd, kvd, kpmd = q.to(cuda), kv.to(cuda), kpm.to(cuda)
    full = Fn.beam_cross_attn(qd, kvd, k_off, sent.to(cuda), n_sent, beam, S, H, 64, kpm=kpmd)
    for i in (0, 3, 7):                                       # the sentence launched alone, and with another beam size
        alone = Fn.beam_cross_attn(qd[i * beam:(i + 1) * beam], kvd, k_off, sent[i:i + 1].to(cuda), n_sent, beam, S, H, 64, kpm=kpmd)
        assert torch.equal(alone, full[i * beam:(i + 1) * beam]), f"sentence {i} alone"
        three = Fn.beam_cross_attn(qd[i * beam + 4:i * beam + 7], kvd, k_off, sent[i:i + 1].to(cuda), n_sent, 3, S, H, 64, kpm=kpmd)
        assert torch.equal(three, full[i * beam + 4:i * beam + 7]), f"three rows of sentence {i} as a beam of 3"
    g = torch.Generator().manual_seed(3)
    perm = torch.cat([i * beam + torch.randperm(beam, generator=g) for i in range(n_sent)]).to(cuda)
    permuted = Fn.beam_cross_attn(qd[perm], kvd, k_off, sent.to(cuda), n_sent, beam, S, H, 64, kpm=kpmd)
    assert torch.equal(permuted, full[perm]), "permuting the rows inside a sentence must permute the bits"
    dup = qd.clone()
    dup[beam + 7] = dup[beam + 2]
    dup[beam + 9] = dup[beam + 2]
    out = Fn.beam_cross_attn(dup, kvd, k_off, sent.to(cuda), n_sent, beam, S, H, 64, kpm=kpmd)
    assert torch.equal(out[beam + 7], out[beam + 2]) and torch.equal(out[beam + 9], out[beam + 2]), "duplicate queries"
    assert torch.equal(out[beam + 2], full[beam + 2])


def test_state_follows_a_recorded_reorder_sequence_on_the_device(cuda):
    """The product's reorder_beam_slots with the real st5_lm_reorder against the row-by-row simulation of tests/beam_slots_reference.py."""
    from speecht5_amd.modules.decoder import BeamSlotState, TransformerDecoder
    n_sent, beam, Tmax, drops = 6, 4, 16, {3: (2,), 7: (0, 4)}
    rows = n_sent * beam
    ident = torch.arange(rows, dtype=torch.int32, device=cuda).unsqueeze(1).expand(rows, Tmax).contiguous()
    st = BeamSlotState([], [ident, torch.empty_like(ident)], Tmax, None, None, None, None,
                       torch.arange(n_sent, dtype=torch.int32, device=cuda), n_sent, beam, 0, None)
    sim = SlotSim(n_sent, beam, Tmax)
    for k, (order, batch_idxs) in enumerate(synthetic_sequence(n_sent, beam, 12, seed=9, drops=drops)):
        sim.step()
        st.t += 1
        bi = torch.from_numpy(batch_idxs).to(cuda) if batch_idxs is not None and k % 2 else None   # (given, or derived from the order)
        TransformerDecoder.reorder_beam_slots(None, st, torch.from_numpy(order).to(cuda), bi)
        sim.reorder(order.tolist())
        sim.check(st.anc.cpu().numpy(), st.sent.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the tiny model: hypotheses of the reference generator
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(cuda):
    _, fx = load_golden("tiny_s2t_beam.pt")
    _, fx_lm = load_golden("tiny_s2t_beam_lm.pt")
    model, args = build_tiny(cuda, torch.float32)
    model.eval()
    from tests.test_lm_fusion_gpu import _tiny_lm
    return model, args, fx, fx_lm, _tiny_lm(fx_lm, cuda), Task().dicts["text"]


def _assert_hyps(hyps, ref_hyps):
    assert len(hyps) == len(ref_hyps)
    for si, (got, ref) in enumerate(zip(hyps, ref_hyps)):
        assert len(got) == len(ref), f"sentence {si}: {len(got)} hypotheses, reference {len(ref)}"
        for hi, (g, r) in enumerate(zip(got, ref)):
            rt = r["tokens"].cpu().tolist()
            rs = float(r["score"])
            assert g["tokens"].cpu().tolist() == rt, f"sentence {si} hypothesis {hi}"
            assert abs(float(g["score"]) - rs) <= SCORE_TOL * max(1.0, abs(rs)), (si, hi, float(g["score"]), rs)
            np.testing.assert_allclose(g["positional_scores"].cpu().numpy(), r["positional_scores"].cpu().numpy(), atol=POS_TOL, rtol=0)


BEAM_CASES = ["beam1", "beam3", "beam3_unnorm_minlen", "beam3_ngram2", "beam2_prefix", "beam3_ctc03", "beam4_ctc05", "beam1_ctc05"]
LM_CASES = ["beam1_lm03", "beam3_lm03", "beam5_lm10", "beam3_lm10_minlen", "beam2_lm03_prefix", "beam1_lm03_shrink", "beam3_lm03_ctc03",
            "beam5_lm03_ctc03"]


def test_the_case_lists_cover_the_goldens(tiny):
    _, _, fx, fx_lm, _, _ = tiny
    assert sorted(BEAM_CASES) == sorted(fx["cases"]) and sorted(LM_CASES) == sorted(fx_lm["cases"])


@pytest.mark.parametrize("name", BEAM_CASES)
def test_slots_hypotheses_equal_reference_generator(cuda, tiny, name):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _, fx, _, _, d = tiny
    case = fx["cases"][name]
    gen = SequenceGenerator([model], d, decode="slots", **case["kw"])
    sample = to_dev(fx["samples"][case["sample"]], cuda)
    prefix = case["prefix"].to(cuda) if case["prefix"] is not None else None
    _assert_hyps(gen.generate([model], sample, prefix_tokens=prefix), case["hyps"])


@pytest.mark.parametrize("name", LM_CASES)
def test_slots_lm_fused_hypotheses_equal_reference_generator(cuda, tiny, name):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _, fx, fx_lm, lm, d = tiny
    case = fx_lm["cases"][name]
    gen = SequenceGenerator([model], d, lm_model=lm, decode="slots", **case["kw"])
    sample = to_dev(fx["samples"][case["sample"]], cuda)
    prefix = case["prefix"].to(cuda) if case["prefix"] is not None else None
    _assert_hyps(gen.generate([model], sample, prefix_tokens=prefix), case["hyps"])


def _ragged_sample(cuda, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    wav = torch.zeros(len(lengths), max(lengths))
    pad = torch.ones(len(lengths), max(lengths), dtype=torch.bool)
    for b, m in enumerate(lengths):
        wav[b, :m] = torch.randn(m, generator=g) * 0.1
        pad[b, :m] = False
    return {"net_input": {"source": wav.to(cuda), "padding_mask": pad.to(cuda)}, "id": torch.arange(len(lengths), device=cuda)}


@pytest.mark.parametrize("kw", [dict(ctc_weight=0.4, ctc_rows=True), dict(ctc_weight=0.4, ctc_rows=True, exact_rows=True),
                                dict(exact_rows=True), dict(ctc_weight=0.3)],
                         ids=["ctc_rows", "ctc_rows_exact_rows", "exact_rows", "ctc_first_sentence"])
def test_slots_equal_concat_under_the_rows_options(cuda, tiny, kw):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _, _, _, _, d = tiny
    sample = _ragged_sample(cuda, [7000, 5200, 6100, 4000], seed=21)
    base = dict(beam_size=3, max_len_b=12, **kw)
    ref = SequenceGenerator([model], d, **base).generate([model], sample)
    got = SequenceGenerator([model], d, decode="slots", **base).generate([model], sample)
    _assert_hyps(got, ref)


def test_slots_ensemble_has_one_state_per_model(cuda, tiny):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _, fx, _, _, d = tiny
    other, _ = build_tiny(cuda, torch.float32)
    other.eval()
    sample = to_dev(fx["samples"]["two"], cuda)
    kw = dict(beam_size=3, max_len_b=10)
    seen = []
    for m in (model, other):
        init = m.decoder.init_beam_slots
        m.decoder.init_beam_slots = (lambda *a, _i=init, **k: seen.append(_i(*a, **k)) or seen[-1])
    try:
        got = SequenceGenerator([model, other], d, decode="slots", **kw).generate([model, other], sample)
    finally:
        for m in (model, other):
            del m.decoder.init_beam_slots
    ref = SequenceGenerator([model, other], d, **kw).generate([model, other], sample)
    assert len(seen) == 2 and seen[0] is not seen[1] and seen[0].kv[0].data_ptr() != seen[1].kv[0].data_ptr()
    _assert_hyps(got, ref)


def test_decode_travels_through_build_generator(cuda, tiny):
    from speecht5_amd.task import SpeechT5Task
    model, args, _, _, _, _ = tiny
    task = SpeechT5Task(args, Task().dicts)
    gen_args = Namespace(beam=1, max_len_a=0, max_len_b=6)
    assert task.build_generator([model], gen_args, extra_gen_cls_kwargs={"decode": "slots"}).decode == "slots"
    assert task.build_generator([model], gen_args).decode == "concat"
    with pytest.raises(ValueError):
        task.build_generator([model], gen_args, extra_gen_cls_kwargs={"decode": "paged"})


# ------------------------------------------------------------------------------------------------------------------------------
# 4. replayed trajectory
# ------------------------------------------------------------------------------------------------------------------------------
def _build_base(dev, dtype):
    from speecht5_amd import functional as Fn
    from speecht5_amd.speecht5 import t5_transformer_base
    from speecht5_amd.task import SpeechT5Task
    Fn.set_compute_dtype(dtype)
    Fn.weight_cache.clear()
    args = Namespace(label_rates=50, sample_rate=16000, speech_odim=80, bert_init=True, use_codebook=False,
                     share_input_output_embed=True, encoder_layerdrop=0.0, decoder_layerdrop=0.0)
    t5_transformer_base(args)
    for k, v in list(vars(args).items()):
        if "dropout" in k and isinstance(v, float):
            setattr(args, k, 0.0)
    task = SpeechT5Task.synthetic(args)
    task.t5_task = "s2t"
    torch.manual_seed(4247)
    return task.build_model(args).to(dev).eval(), task.target_dictionary


def _build_tiny_large(dev, dtype):
    from speecht5_amd import functional as Fn
    from tests.test_large_gpu import _build
    Fn.weight_cache.clear()
    model, args, _ = _build(dev, dtype)
    assert args.decoder_normalize_before
    return model.eval(), Task().dicts["text"]


def _record_concat(model, d, sample, beam, max_len_b, plan):
    """One `concat` generate(); per step (the token prefix fed, reorder_state or None, batch_idxs or None) and the log-probabilities
    the decoder returned.  `plan` {original sentence: step}: from that step on the sentence's hypotheses all close with </s>, so it
    finishes early; no other hypothesis closes before the length limit, whatever the model says."""
    from speecht5_amd.sequence_generator import BeamSearch, SequenceGenerator
    rec, lprobs, pending = [], [], {"order": None, "bidx": None}

    class ForcedEos(BeamSearch):
        def step(self, step, lp, scores, prev_output_tokens=None, original_batch_idxs=None):
            lp = lp.clone()
            if step < max_len_b:                              # (the last step may only close: the generator has seen to that)
                lp[:, :, d.eos()] = -float("inf")
                for i, ob in enumerate(original_batch_idxs.tolist()):
                    if ob in plan and step >= plan[ob]:
                        lp[i, :, d.eos()] = 0.0
            return super().step(step, lp, scores, prev_output_tokens, original_batch_idxs)

        def prune_sentences(self, batch_idxs):
            pending["bidx"] = batch_idxs.clone()

    gen = SequenceGenerator([model], d, beam_size=beam, max_len_b=max_len_b, search_strategy=ForcedEos(d))
    ens = gen.model
    fd, ro = ens.forward_decoder, ens.reorder_incremental_state

    def reorder(states, order):
        pending["order"] = order.clone()
        return ro(states, order)

    def forward_decoder(tokens, encoder_outs, states, temperature=1.0):
        out = fd(tokens, encoder_outs, states, temperature)
        rec.append((tokens.clone(), pending["order"], pending["bidx"]))
        pending["order"], pending["bidx"] = None, None
        lprobs.append(out[0].float().clone())
        return out

    ens.reorder_incremental_state, ens.forward_decoder = reorder, forward_decoder
    try:
        hyps = gen.generate([model], sample)
    finally:
        del ens.reorder_incremental_state, ens.forward_decoder
    return rec, lprobs, hyps


def _replay(model, d, sample, rec, beam, mode):
    from speecht5_amd.sequence_generator import EnsembleModel
    ens = EnsembleModel([model])
    net_input = sample["net_input"]
    bsz = net_input["source"].shape[0]
    with torch.no_grad():
        encoder_outs = ens.forward_encoder(net_input)
        states = [{}]
        if mode == "slots":
            ens.init_beam_slots(states, bsz, beam, len(rec) + 2, encoder_outs)
        else:
            new_order = torch.arange(bsz, device=net_input["source"].device).view(-1, 1).repeat(1, beam).view(-1)
            encoder_outs = ens.reorder_encoder_out(encoder_outs, new_order)
        out = []
        for tokens, order, bidx in rec:
            if order is not None:
                if mode == "slots":
                    ens.reorder_beam_slots(states, order, bidx)
                else:
                    ens.reorder_incremental_state(states, order)
                    encoder_outs = ens.reorder_encoder_out(encoder_outs, order)
            out.append(ens.forward_decoder(tokens, encoder_outs, states, 1.0)[0].float().clone())
    return out


def _worst(a, b):
    return max(float((x - y).abs().max()) for x, y in zip(a, b))


def _trajectory(cuda, build, name, lengths, plan, min_steps):
    beam, max_len_b = 10, 44
    model, d = build(cuda, torch.float32)
    sample = _ragged_sample(cuda, lengths, seed=13)
    rec, ref, hyps = _record_concat(model, d, sample, beam, max_len_b, plan)
    rows = [t.shape[0] for t, _, _ in rec]
    assert len(rec) >= min_steps and min(rows) < rows[0], f"{len(rec)} steps, rows per step {rows}: no sentence finished early"
    assert any(b is not None for _, _, b in rec)
    again = _replay(model, d, sample, rec, beam, "concat")
    assert _worst(again, ref) <= 1e-6, "the replay driver does not reproduce the concat run it was recorded from"
    slots = _replay(model, d, sample, rec, beam, "slots")
    e32 = _worst(slots, ref)
    _report(f"{name} fp32: {len(rec)} steps, rows {rows[0]} -> {rows[-1]}, S = {int((~sample['net_input']['padding_mask']).sum(1).max()) // 320}"
            f" frames at most; max |lprobs(slots) - lprobs(concat)| = {e32:.3e} (bar {POS_TOL})")
    del model
    model16, _ = build(cuda, torch.bfloat16)
    c16 = _worst(_replay(model16, d, sample, rec, beam, "concat"), ref)
    s16 = _worst(_replay(model16, d, sample, rec, beam, "slots"), ref)
    _report(f"{name} bf16 against the fp32 concat run on the same trajectory: concat {c16:.3e}, slots {s16:.3e}, "
            f"ratio {s16 / c16:.3f} (margin {BF16_MARGIN})")
    assert e32 <= POS_TOL, e32
    assert s16 <= BF16_MARGIN * c16, (s16, c16)


def test_base_size_replayed_trajectory(cuda):
    """Measured on MI355X: profiles/beam_slots_parity.txt."""
    lengths = [32000, 17000, 25000, 21000, 30000, 16000, 28000, 19000]           # 1 ... 2 s; S is the padded maximum, 99 frames: the split path (one range: tiny-Large below)
    _trajectory(cuda, _build_base, "Base", lengths, plan={2: 5, 5: 17}, min_steps=40)


def test_tiny_large_pre_ln_replayed_trajectory(cuda):
    lengths = [7000, 4200, 6100, 5000, 6600, 4000, 5600, 4800]
    _trajectory(cuda, _build_tiny_large, "tiny-Large (pre-LN)", lengths, plan={1: 4, 6: 11}, min_steps=40)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. no copies
# ------------------------------------------------------------------------------------------------------------------------------
def test_no_key_value_or_encoder_tensor_moves(cuda, tiny):
    from speecht5_amd.sequence_generator import EnsembleModel, SequenceGenerator
    model, _, _, _, _, d = tiny
    sample = _ragged_sample(cuda, [7000, 5200, 6100, 4000], seed=23)
    states, first, calls = [], {}, []
    init, step = model.decoder.init_beam_slots, model.decoder._extract_features_beam_slots

    def pointers(st):
        return [t.data_ptr() for t in st.kv] + [t.data_ptr() for t, _ in st.xkv] + [st.enc_rows.data_ptr(), st.kpm.data_ptr()]

    def counted_init(*a, **k):
        states.append(init(*a, **k))
        return states[-1]

    def counted_step(prev, st, *a, **k):
        first.setdefault("ptrs", pointers(st))
        first["last"] = pointers(st)
        first["steps"] = first.get("steps", 0) + 1
        return step(prev, st, *a, **k)

    enc_reorder, ens_reorder = model.encoder.reorder_encoder_out, EnsembleModel.reorder_encoder_out
    model.decoder.init_beam_slots, model.decoder._extract_features_beam_slots = counted_init, counted_step
    model.encoder.reorder_encoder_out = lambda *a, **k: calls.append("encoder") or enc_reorder(*a, **k)
    EnsembleModel.reorder_encoder_out = lambda self, *a, **k: calls.append("ensemble") or ens_reorder(self, *a, **k)
    try:
        hyps = SequenceGenerator([model], d, beam_size=4, max_len_b=12, ctc_weight=0.3, ctc_rows=True,
                                 decode="slots").generate([model], sample)
    finally:
        del model.decoder.init_beam_slots, model.decoder._extract_features_beam_slots, model.encoder.reorder_encoder_out
        EnsembleModel.reorder_encoder_out = ens_reorder
    assert len(hyps) == 4 and len(states) == 1 and first["steps"] >= 5
    assert first["ptrs"] == first["last"] == pointers(states[0]), "a K/V buffer or the encoder rows moved during the generate"
    assert calls == [], f"reorder_encoder_out was called: {calls}"
    assert states[0].enc_rows.shape[0] == 4 * states[0].S, "the encoder rows are kept once per sentence, not per hypothesis"
