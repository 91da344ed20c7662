"""Decode loop of generate_speech_batch / synthesize_batch with the step index on the device (decode="device") and replayed from a
HIP graph (decode="graph"); the mechanism (step program, layer sequence, replay loop) is step_program.py.

The step: the Tacotron pre-net (dropout always on, its seeds read from a per-step table), the scaled positional row and the speaker
integration, the decoder layers with the cross-attention's record column, feat_out | prob_out in one product, and the step tail,
which advances the counter.  Step-invariant work is done once per call: the speaker embedding's normalisation, the cross-attention
K|V projection, the key-padding bytes, the workspaces and the compute-dtype weight images.  Every buffer the graph has baked in
belongs to the DeviceDecode object, which outlives the graph.
"""
import torch

from . import functional as Fn
from .step_program import (GRAPH_WARMUP_STEPS, StepProgram, append_layers, decode_stream, on_decode_stream,  # noqa: F401
                           replay_schedule, run_steps)

DECODE_MODES = ("eager", "device", "graph")


def unsupported_reason(model, spkembs):
    """Why this model cannot run the device-stepped decode (None when it can)."""
    if model.training:
        return "the model is in training mode (dropout / LayerDrop semantics of the training forward)"
    layers = list(model.decoder.layers)
    if any(l.encoder_attn is None for l in layers):
        return "a decoder layer has no encoder attention"
    a = layers[0].self_attn
    if a.head_dim != 64:
        return f"head_dim is {a.head_dim}; the one-query cross-attention kernel is built for head_dim 64"
    if spkembs is not None and not hasattr(model.speech_decoder_prenet, "spkembs_layer"):
        return "speaker embeddings are given but spk_embed_integration_type is not 'pre'"
    return None


class DeviceDecode:
    """Buffers and launch sequence of one call's decode steps."""

    def __init__(self, model, encoder_out, T_in, spkembs, need_attn, text, **kwargs):
        from .modules.multihead_attention import _mask_bytes
        from .speecht5 import tts_row_limits
        r = model.reduction_factor
        self.threshold, self.minlen, self.maxlen, self.cap = tts_row_limits(T_in, r, text, **kwargs)
        cap = self.cap
        enc = encoder_out["encoder_out"][0]
        S, B = enc.size(0), enc.size(1)
        dev, dtype = enc.device, Fn.compute_dtype()
        post, pre, dec = model.speech_decoder_postnet, model.speech_decoder_prenet, model.decoder
        odim = post.odim
        C = model.args.decoder_embed_dim
        layers = list(dec.layers)
        H = layers[0].self_attn.num_heads
        hd = C // H
        self.B, self.r, self.odim = B, r, odim
        prog = self.prog = StepProgram(dev, dtype, B)
        new, lin = prog.new, prog.lin
        i32 = dict(dtype=torch.int32, device=dev)
        self.counter = torch.zeros(1, **i32)
        self.minlen_d, self.maxlen_d = torch.tensor(self.minlen, **i32), torch.tensor(self.maxlen, **i32)
        self.done, self.steps, self.active = torch.zeros(B, **i32), torch.zeros(B, **i32), torch.zeros(1, **i32)
        self.mel_rec = new(B, cap * r, odim, dt=torch.float32)
        self.prob_rec = new(B, cap * r, dt=torch.float32)
        self.rec = new(B, len(layers), H, cap, S, dt=torch.float32) if need_attn else None
        self.nxt = torch.zeros(B, odim, dtype=dtype, device=dev)
        self.host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        self.event = torch.cuda.Event()
        anc = torch.arange(B, **i32).unsqueeze(1).expand(B, cap).contiguous()
        attn_ws = Fn.lm_decode_attn_ws(B, cap, H, hd, dev)

        # ---- pre-net: Tacotron pre-net (dropout always on), Linear, scaled positional row, speaker integration ----
        inl, spe = pre.decoder_prenet[0], pre.decoder_prenet[1]
        tac = inl[0]
        p_drop = float(tac.dropout_rate)
        n_seeds = len(tac.prenet) if p_drop > 0 else 0
        self.seed_slots = self.seed_table = None
        if n_seeds:
            self.seed_table = Fn.next_seeds(cap * n_seeds).view(cap, n_seeds).to(dev)   # (step-major: the order a host loop would draw)
            self.seed_slots = self.seed_table[0].clone()
        x = self.nxt
        for k, blk in enumerate(tac.prenet):
            seed = ((1 << 63) | (self.seed_slots.data_ptr() + 8 * k)) if n_seeds else 0
            x = lin(x, [blk[0].weight], [blk[0].bias], new(B, blk[0].weight.shape[0]), act=Fn.ACT_RELU, dropout_p=p_drop, seed=seed)
        x = lin(x, [inl[1].weight], [inl[1].bias], new(B, C))
        table = spe.pe(cap, dev)
        alpha = spe.alpha.detach()
        if spkembs is not None:
            lin_s = pre.spkembs_layer[0]
            cat = new(B, lin_s.weight.shape[1])
            cat[:, C:] = Fn.as_compute(torch.nn.functional.normalize(spkembs.float()).contiguous())   # once, not per step
            prog.add(lambda x=x: Fn.tts_pe_add_step(x, table, alpha, self.counter, cat))
            x = lin(cat, [lin_s.weight], [lin_s.bias], new(B, C), act=Fn.ACT_RELU)
        else:
            y = new(B, C)
            prog.add(lambda x=x, y=y: Fn.tts_pe_add_step(x, table, alpha, self.counter, y))
            x = y

        # ---- decoder layers ----
        enc_rows = Fn.as_compute(enc.transpose(0, 1).contiguous()).view(B * S, -1)
        pad = encoder_out["encoder_padding_mask"][0] if len(encoder_out["encoder_padding_mask"]) > 0 else None
        kpm = _mask_bytes(pad) if pad is not None else None
        cross_ws = Fn.decode_cross_attn_ws(B, S, H, hd, dev)
        self.slots = [new(B, cap, 2 * C) for _ in layers]
        self.kvp = [Fn.linear(enc_rows, [ca.k_proj.weight, ca.v_proj.weight], [ca.k_proj.bias, ca.v_proj.bias])   # step-invariant
                    for ca in (l.encoder_attn for l in layers)]
        recs = [self.rec[:, li] if self.rec is not None else None for li in range(len(layers))]

        def self_attn(q, slots, ctx, H, hd):
            Fn.lm_decode_attn_dev(q, slots, anc, self.counter, 1, cap, H, hd, ctx, attn_ws)

        def cross_attn(li, q, ctx):
            Fn.decode_cross_attn_step(q, self.kvp[li], 0, S, H, hd, ctx, self.counter, cap, kpm=kpm, rec=recs[li], ws=cross_ws)

        x = append_layers(prog, x, layers, self.slots, cap, self.counter, self_attn, cross_attn, dec.layer_norm)

        # ---- feat_out | prob_out in one launch with fp32 output (no cast kernel), then the step tail ----
        nf = post.feat_out.weight.shape[0] + post.prob_out.weight.shape[0]
        y = lin(x, [post.feat_out.weight, post.prob_out.weight], [post.feat_out.bias, post.prob_out.bias], new(B, nf, dt=torch.float32),
                out_f32=True)
        prog.add(lambda: Fn.tts_step_tail_dev(y, r, odim, self.minlen_d, self.maxlen_d, self.done, self.steps, self.counter,
                                              self.threshold, self.mel_rec, self.prob_rec, self.nxt, self.active, self.seed_table,
                                              self.seed_slots))
        prog.finish()

    def poll(self):
        """Rows still running after the steps enqueued so far (one host read, as the eager loop's poll)."""
        self.host.copy_(self.active, non_blocking=True)
        self.event.record()
        self.event.synchronize()
        return int(self.host[0])


def decode_rows(model, source, src_tokens, spkembs, padding_mask, need_attn, mode, **kwargs):
    """_decode_rows of T5TransformerModel in "device" / "graph" mode: the same five results."""
    assert mode in ("device", "graph")
    why = unsupported_reason(model, spkembs)
    if why is not None:
        raise RuntimeError(f"generate_speech_batch(decode={mode!r}) is not available: {why}")
    encoder_out, T_in = model._encode_rows(source, src_tokens, padding_mask)
    stats = {"polls": 0, "device_steps": 0, "graph_replays": 0}
    with on_decode_stream(model, encoder_out["encoder_out"][0].device, mode) as caller:
        st = DeviceDecode(model, encoder_out, T_in, spkembs, need_attn, source is None, **kwargs)
        run_steps(st.prog.step, st.cap, mode, model.TTS_POLL_STEPS, lambda: st.poll() == 0, stats,
                  profile=bool(getattr(model, "tts_profile", False)))
    model.tts_polls = stats["polls"]
    model.tts_device_steps = stats["device_steps"]
    model.tts_graph_replays = stats["graph_replays"]
    model.tts_stats = stats
    steps = st.steps.tolist()
    if caller is not None:
        for t in (st.mel_rec, st.prob_rec, st.rec):
            if t is not None:
                t.record_stream(caller)
    return st.mel_rec, st.prob_rec, st.rec, steps, T_in
