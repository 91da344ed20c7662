"""Beam search over a slot cache, the parts that need no GPU (speecht5_amd/sequence_generator.py decode="slots",
TransformerDecoder.reorder_beam_slots, tests/beam_slots_reference.py):
1. the fp64 restatement of st5_beam_cross_attn's contract against a brute-force form on K|V replicated per hypothesis row, and the
   planted faults that this comparison must catch;
2. the host bookkeeping -- the `sent` map through successive shrinks and the ancestry table -- against a row-by-row simulation of a
   seeded reorder / shrink sequence (the product's reorder_beam_slots with st5_lm_reorder restated in numpy);
3. the constructor contract of SequenceGenerator(decode=...)."""
import numpy as np
import pytest
import torch

from tests.beam_slots_reference import (FAULTS, SlotSim, beam_cross_attn_brute, beam_cross_attn_ref, reorder_ref, synthetic_sequence)
from tests.fake_seq_model import FakeSeqModel
from tests.util import Task


def _case(seed, n_sent=4, n_live=3, beam=3, S=11, H=2, k_off=16, pad_cols=24, with_kpm=True):
    g = torch.Generator().manual_seed(seed)
    C = H * 64
    ld = k_off + 2 * C + pad_cols
    kv = torch.randn(n_sent * S, ld, generator=g, dtype=torch.float64)
    q = torch.randn(n_live * beam, C, generator=g, dtype=torch.float64) * 1.5
    sent = torch.randperm(n_sent, generator=g)[:n_live].tolist()
    kpm = None
    if with_kpm:
        kpm = torch.zeros(n_sent, S, dtype=torch.bool)
        for s in range(n_sent):
            kpm[s, S - 1 - (s % 4):] = True              # ragged padded tails, at least one padded key per sentence
    return dict(q=q, kv=kv, k_off=k_off, sent=sent, n_sent=n_sent, beam=beam, S=S, H=H, kpm=kpm)


@pytest.mark.parametrize("seed,kw", [(0, {}), (1, dict(beam=1)), (2, dict(n_sent=6, n_live=6, beam=5, S=70)), (3, dict(with_kpm=False, k_off=0))])
def test_restatement_equals_brute_force(seed, kw):
    c = _case(seed, **kw)
    ctx, probs = beam_cross_attn_ref(**c)
    bctx, bprobs = beam_cross_attn_brute(**c)
    torch.testing.assert_close(ctx, bctx, atol=1e-12, rtol=0)
    torch.testing.assert_close(probs, bprobs, atol=1e-12, rtol=0)
    if c["kpm"] is not None:
        rows_sent = torch.tensor(c["sent"]).repeat_interleave(c["beam"])
        ex = c["kpm"][rows_sent].unsqueeze(1).expand_as(probs)
        assert (probs[ex] == 0).all(), "an excluded key gets exactly 0"
    torch.testing.assert_close(probs.sum(-1), torch.ones(probs.shape[:2], dtype=torch.float64), atol=1e-12, rtol=0)


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_faults_are_caught(fault):
    c = _case(7)
    bctx, bprobs = beam_cross_attn_brute(**c)
    ctx, probs = beam_cross_attn_ref(**c, fault=fault)
    err = max(float((ctx - bctx).abs().max()), float((probs - bprobs).abs().max()))
    assert err > 1e-3, (fault, err)


def test_bad_sentence_entry_gives_nan_in_its_rows_only():
    c = _case(11)
    good_ctx, good_probs = beam_cross_attn_ref(**c)
    for bad in (-1, c["n_sent"]):
        d = dict(c, sent=[c["sent"][0], bad, c["sent"][2]])
        ctx, probs = beam_cross_attn_ref(**d)
        b = c["beam"]
        assert torch.isnan(ctx[b:2 * b]).all() and torch.isnan(probs[b:2 * b]).all()
        keep = torch.cat([torch.arange(0, b), torch.arange(2 * b, 3 * b)])
        assert torch.equal(ctx[keep], good_ctx[keep]) and torch.equal(probs[keep], good_probs[keep])


# ------------------------------------------------------------------------------------------------------------------------------
# 2. host bookkeeping: the product's reorder_beam_slots over a seeded reorder / shrink sequence
# ------------------------------------------------------------------------------------------------------------------------------
def _cpu_state(n_sent, beam, Tmax):
    from speecht5_amd.modules.decoder import BeamSlotState
    rows = n_sent * beam
    ident = torch.arange(rows, dtype=torch.int32).unsqueeze(1).expand(rows, Tmax).contiguous()
    bufs = [ident, torch.empty(rows, Tmax, dtype=torch.int32)]
    return BeamSlotState([], bufs, Tmax, None, None, None, None, torch.arange(n_sent, dtype=torch.int32), n_sent, beam, 0, None)


def _lm_reorder_numpy(anc, order, t, out):
    n = order.numel()
    out[:n] = torch.from_numpy(reorder_ref(anc.numpy(), order.numpy(), int(t)))
    return out[:n]


@pytest.mark.parametrize("give_batch_idxs", [True, False])
@pytest.mark.parametrize("n_sent,beam,drops", [(5, 3, {2: (1,), 5: (0, 3), 8: (1,)}), (4, 1, {1: (0,), 2: (2,)}), (3, 4, {})])
def test_sent_map_and_ancestry_follow_a_recorded_sequence(monkeypatch, n_sent, beam, drops, give_batch_idxs):
    from speecht5_amd import functional as Fn
    from speecht5_amd.modules.decoder import TransformerDecoder
    monkeypatch.setattr(Fn, "lm_reorder", _lm_reorder_numpy)
    steps, Tmax = 11, 14
    st = _cpu_state(n_sent, beam, Tmax)
    sim = SlotSim(n_sent, beam, Tmax)
    ptrs = [b.data_ptr() for b in st.bufs]
    for order, batch_idxs in synthetic_sequence(n_sent, beam, steps, seed=3, drops=drops):
        sim.step()
        st.t += 1                                             # (what a decode step does to the state)
        sim.check(st.anc.numpy(), st.sent.numpy())
        TransformerDecoder.reorder_beam_slots(None, st, torch.from_numpy(order),
                                              torch.from_numpy(batch_idxs) if batch_idxs is not None and give_batch_idxs else None)
        sim.reorder(order.tolist())
        assert st.rows == len(order) and st.sent.numel() * beam == len(order)
        sim.check(st.anc.numpy(), st.sent.numpy())
        assert st.anc.data_ptr() in ptrs, "the table ping-pongs between its two buffers"
    assert st.sent.numel() == n_sent - sum(len(v) for v in drops.values())


# ------------------------------------------------------------------------------------------------------------------------------
# 3. constructor contract
# ------------------------------------------------------------------------------------------------------------------------------
def test_default_decode_is_concat():
    from speecht5_amd.sequence_generator import SequenceGenerator
    d = Task().dicts["text"]
    model = FakeSeqModel(len(d)).eval()
    assert SequenceGenerator([model], d, beam_size=2).decode == "concat"
    assert SequenceGenerator([model], d, beam_size=2, decode="concat").decode == "concat"


def test_slots_with_a_decoder_without_the_slot_api_is_refused():
    from speecht5_amd.sequence_generator import SequenceGenerator
    d = Task().dicts["text"]
    model = FakeSeqModel(len(d)).eval()
    with pytest.raises(ValueError, match="slots"):
        SequenceGenerator([model], d, beam_size=2, decode="slots")


def test_unknown_decode_value_is_refused():
    from speecht5_amd.sequence_generator import SequenceGenerator
    d = Task().dicts["text"]
    model = FakeSeqModel(len(d)).eval()
    with pytest.raises(ValueError, match="decode"):
        SequenceGenerator([model], d, beam_size=2, decode="slot")


def test_decoders_the_slot_kernels_do_not_cover_are_refused_at_construction():
    """head dims other than 64 (cross-attention), more than 64 heads, or an encoder attention in only some layers: ValueError from
    check_beam_slots, which the generator's constructor calls -- not ST5_ERR_ARG at the first decode step."""
    from types import SimpleNamespace as NS
    from speecht5_amd.modules.decoder import TransformerDecoder
    from speecht5_amd.sequence_generator import SequenceGenerator

    def dec(hd=64, H=12, cross=(True, True)):
        attn = NS(head_dim=hd, num_heads=H)
        return NS(layers=[NS(self_attn=attn, encoder_attn=attn if c else None) for c in cross])

    TransformerDecoder.check_beam_slots(dec())
    TransformerDecoder.check_beam_slots(dec(cross=(False, False)))
    for bad in (dec(hd=80), dec(hd=32), dec(H=65), dec(cross=(True, False))):
        with pytest.raises(ValueError, match="slots"):
            TransformerDecoder.check_beam_slots(bad)
    d = Task().dicts["text"]
    model = FakeSeqModel(len(d)).eval()
    model.decoder.init_beam_slots = lambda *a, **k: None
    model.decoder.check_beam_slots = lambda: TransformerDecoder.check_beam_slots(dec(hd=80))
    with pytest.raises(ValueError, match="80"):
        SequenceGenerator([model], d, beam_size=2, decode="slots")
