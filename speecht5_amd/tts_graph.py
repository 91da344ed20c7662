"""Decode loop of generate_speech_batch / synthesize_batch with the step index on the device (decode="device") and replayed from a
HIP graph (decode="graph").

One decode step is a fixed sequence of kernel launches on caller-owned buffers: every GEMM of the step runs on the weight-streaming
skinny-M kernel (csrc/decode_gemm.hip), the self-attention K|V projection writes slot `counter` of the cache through that kernel's
device-side output offset, and the self-attention, the cross-attention's record column, the positional row, the pre-net's dropout
seeds and the step tail all read ONE int32 counter in device memory (steps completed so far), which the tail advances.  Nothing in
the step depends on a host value, allocates, or builds a weight image, so the same launch sequence can be enqueued kernel by
kernel ("device": the warm-up and debugging form) or captured once and replayed ("graph").  Step-invariant work is done once per
call: the speaker embedding's normalisation, the cross-attention K|V projection, the key-padding bytes, the workspaces and the
compute-dtype weight images.

The captured step has no forked stream and no parallel branch: every launch goes to the one capturing stream.  No library entry
with a per-stream table is part of the step (st5_gemm, whose split-K slabs are per stream, is not called), and every buffer the
graph has baked in belongs to the DeviceDecode object, which outlives the graph.
"""
import gc

import torch

from . import functional as Fn
from . import hip

DECODE_MODES = ("eager", "device", "graph")
GRAPH_WARMUP_STEPS = 1      # steps run kernel by kernel before the capture (everything first-use happens in them)


def replay_schedule(cap, poll_steps, eager_steps=GRAPH_WARMUP_STEPS):
    """The decode loop as groups between two polls of the active-row count: a list of (first, n_eager, n_replay, poll).  A group runs
    the steps first .. first + n_eager + n_replay - 1 (1-based, in order): n_eager of them kernel by kernel, then n_replay graph
    replays; `poll` says whether the host reads the active count behind the group's last step -- exactly where the eager loop polls
    (idx % poll_steps == 0 and idx < cap).  The groups cover 1 .. cap once and never pass cap; a loop that finds no active row at a
    poll stops behind that group, where the eager loop stops."""
    assert cap >= 1 and poll_steps >= 1 and eager_steps >= 0
    groups, idx, left = [], 1, eager_steps
    while idx <= cap:
        last = min(cap, ((idx - 1) // poll_steps + 1) * poll_steps)
        n = last - idx + 1
        ne = min(left, n)
        left -= ne
        groups.append((idx, ne, n - ne, last % poll_steps == 0 and last < cap))
        idx = last + 1
    return groups


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
        new = lambda *shape, dt=dtype: torch.empty(*shape, dtype=dt, device=dev)   # noqa: E731
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
        stats = new(2 * B, dt=torch.float32)

        weights = []     # (every compute-dtype weight image of the step: held here, so the weight cache cannot drop one mid-call)

        def W(ws_):
            w = Fn.fused_weight(list(ws_), dtype)
            weights.append(w)
            return w

        def bias(bs):
            bs = list(bs)
            return None if any(b is None for b in bs) else Fn.fused_bias(bs)

        ops = []         # the step: zero-argument launches in order
        shapes = []      # (N, K) of every skinny product, for the shared workspace

        def lin(x, ws_, bs, out, **epi):
            w, b = W(ws_), bias(bs)
            shapes.append(tuple(w.shape))
            ops.append(lambda: Fn.linear_skinny(x, w, b, out=out, ws=self.ws, **epi))
            return out

        def norm(ln, x, y):
            ops.append(lambda: Fn.layer_norm_into(x, ln.weight, ln.bias, ln.eps, y, stats))
            return y

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
            ops.append(lambda x=x: Fn.tts_pe_add_step(x, table, alpha, self.counter, cat))
            x = lin(cat, [lin_s.weight], [lin_s.bias], new(B, C), act=Fn.ACT_RELU)
        else:
            y = new(B, C)
            ops.append(lambda x=x, y=y: Fn.tts_pe_add_step(x, table, alpha, self.counter, y))
            x = y

        # ---- decoder layers ----
        enc_rows = Fn.as_compute(enc.transpose(0, 1).contiguous()).view(B * S, -1)
        pad = encoder_out["encoder_padding_mask"][0] if len(encoder_out["encoder_padding_mask"]) > 0 else None
        kpm = _mask_bytes(pad) if pad is not None else None
        cross_ws = Fn.decode_cross_attn_ws(B, S, H, hd, dev)
        self.slots, self.kvp = [], []
        for li, layer in enumerate(layers):
            nb = layer.normalize_before
            sa, ca = layer.self_attn, layer.encoder_attn
            slots = new(B, cap, 2 * C)
            kvp = Fn.linear(enc_rows, [ca.k_proj.weight, ca.v_proj.weight], [ca.k_proj.bias, ca.v_proj.bias])   # step-invariant
            self.slots.append(slots)
            self.kvp.append(kvp)
            rec_l = self.rec[:, li] if self.rec is not None else None
            # self-attention
            h = norm(layer.self_attn_layer_norm, x, new(B, C)) if nb else x
            q = lin(h, [sa.q_proj.weight], [sa.q_proj.bias], new(B, C))
            lin(h, [sa.k_proj.weight, sa.v_proj.weight], [sa.k_proj.bias, sa.v_proj.bias], slots, step=self.counter, step_stride=2 * C,
                step_cap=cap, out_ld=cap * 2 * C)
            ctx = new(B, C)
            ops.append(lambda q=q, slots=slots, ctx=ctx: Fn.lm_decode_attn_dev(q, slots, anc, self.counter, 1, cap, H, hd, ctx, attn_ws))
            x = lin(ctx, [sa.out_proj.weight], [sa.out_proj.bias], new(B, C), residual=x)
            if not nb:
                x = norm(layer.self_attn_layer_norm, x, new(B, C))
            # cross-attention
            h = norm(layer.encoder_attn_layer_norm, x, new(B, C)) if nb else x
            q = lin(h, [ca.q_proj.weight], [ca.q_proj.bias], new(B, C))
            ctx = new(B, C)
            ops.append(lambda q=q, kvp=kvp, ctx=ctx, rec_l=rec_l: Fn.decode_cross_attn_step(q, kvp, 0, S, H, hd, ctx, self.counter, cap,
                                                                                          kpm=kpm, rec=rec_l, ws=cross_ws))
            x = lin(ctx, [ca.out_proj.weight], [ca.out_proj.bias], new(B, C), residual=x)
            if not nb:
                x = norm(layer.encoder_attn_layer_norm, x, new(B, C))
            # feed-forward
            h = norm(layer.final_layer_norm, x, new(B, C)) if nb else x
            f = lin(h, [layer.fc1.weight], [layer.fc1.bias], new(B, layer.fc1.weight.shape[0]), act=layer.act)
            x = lin(f, [layer.fc2.weight], [layer.fc2.bias], new(B, C), residual=x)
            if not nb:
                x = norm(layer.final_layer_norm, x, new(B, C))
        if dec.layer_norm is not None:
            x = norm(dec.layer_norm, x, new(B, C))

        # ---- feat_out | prob_out in one launch with fp32 output (no cast kernel), then the step tail ----
        nf = post.feat_out.weight.shape[0] + post.prob_out.weight.shape[0]
        y = lin(x, [post.feat_out.weight, post.prob_out.weight], [post.feat_out.bias, post.prob_out.bias], new(B, nf, dt=torch.float32),
                out_f32=True)
        ops.append(lambda: Fn.tts_step_tail_dev(y, r, odim, self.minlen_d, self.maxlen_d, self.done, self.steps, self.counter,
                                                self.threshold, self.mel_rec, self.prob_rec, self.nxt, self.active, self.seed_table,
                                                self.seed_slots))
        nbytes = max(int(hip.lib().st5_gemm_skinny_ws_bytes(N, K)) for N, K in shapes)
        self.ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
        self.ops, self.weights = ops, weights

    def step(self):
        for op in self.ops:
            op()

    def poll(self):
        """Rows still running after the steps enqueued so far (one host read, as the eager loop's poll)."""
        self.host.copy_(self.active, non_blocking=True)
        self.event.record()
        self.event.synchronize()
        return int(self.host[0])

    def run(self, mode, poll_steps, stats, profile=False):
        """The loop: `stats` receives polls / device steps / graph replays.  profile: HIP events around every group of steps, so that
        the time of the steps themselves (stats["step_ms"]: device time from the first launch of a group to the end of its last kernel,
        summed over the groups, the capture excluded) can be told from the call's set-up and capture (stats["capture_s"], host clock)."""
        import time
        cap = self.cap
        graph = None
        spans = []
        try:
            for _first, n_eager, n_replay, poll in replay_schedule(cap, poll_steps, GRAPH_WARMUP_STEPS if mode == "graph" else cap):
                if n_replay and graph is None:
                    for _ in range(n_eager):        # (the warm-up steps in front of the capture)
                        self.step()
                        stats["device_steps"] += 1
                    n_eager = 0
                    t0 = time.perf_counter()
                    graph = self._capture()
                    stats["capture_s"] = time.perf_counter() - t0
                if profile:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                for _ in range(n_eager):
                    self.step()
                    stats["device_steps"] += 1
                for _ in range(n_replay):
                    graph.replay()
                    stats["graph_replays"] += 1
                if profile:
                    e1.record()
                    spans.append((e0, e1, n_eager + n_replay))
                if poll:
                    stats["polls"] += 1
                    if self.poll() == 0:
                        break
        finally:
            if graph is not None:
                # released here, with nothing in flight: a CUDAGraph must never be destroyed inside a later capture
                torch.cuda.current_stream().synchronize()
                graph.reset()
                del graph
        if profile and spans:
            torch.cuda.current_stream().synchronize()
            stats["step_ms"] = sum(a.elapsed_time(b) for a, b, _ in spans)
            stats["steps_timed"] = sum(n for _, _, n in spans)

    def _capture(self):
        stream = torch.cuda.current_stream()
        stream.synchronize()
        gc.collect()    # (a graph object freed by the cyclic collector DURING a capture aborts the process)
        graph = torch.cuda.CUDAGraph()
        # capture_begin / capture_end directly: the torch.cuda.graph context would also empty the allocator's cache; the step allocates
        # nothing, so the capture needs no memory pool of its own
        graph.capture_begin(capture_error_mode="thread_local")
        try:
            self.step()
        except BaseException as first:
            try:                       # the capture is invalid by now and ending it may fail in turn: the step's error is the cause
                graph.capture_end()
            except Exception:
                pass
            raise first
        graph.capture_end()
        return graph


def decode_stream(model, device):
    """The stream the graph mode runs on: the caller's current stream, or, when that is the legacy NULL stream (which cannot
    capture), ONE side stream per model and device, kept for the model's lifetime as graph.StepGraph keeps its stream -- the caching
    allocator keeps its blocks per stream, so a fresh stream per call could never reuse what the previous call freed."""
    cur = torch.cuda.current_stream(device)
    if cur != torch.cuda.default_stream(device):
        return cur
    streams = model.__dict__.setdefault("_tts_graph_streams", {})
    key = (device.type, device.index)
    if key not in streams:
        streams[key] = torch.cuda.Stream(device=device)
    return streams[key]


def decode_rows(model, source, src_tokens, spkembs, padding_mask, need_attn, mode, **kwargs):
    """_decode_rows of T5TransformerModel in "device" / "graph" mode: the same five results."""
    assert mode in ("device", "graph")
    why = unsupported_reason(model, spkembs)
    if why is not None:
        raise RuntimeError(f"generate_speech_batch(decode={mode!r}) is not available: {why}")
    encoder_out, T_in = model._encode_rows(source, src_tokens, padding_mask)
    stats = {"polls": 0, "device_steps": 0, "graph_replays": 0}
    device = encoder_out["encoder_out"][0].device
    cur = torch.cuda.current_stream(device)
    # "graph" never runs on the legacy NULL stream; the caller's stream is ordered in front of the loop and behind it, so for the
    # caller it behaves like work on its own stream
    side = decode_stream(model, device) if mode == "graph" else cur
    if side != cur:
        side.wait_stream(cur)
    with torch.cuda.stream(side):
        st = DeviceDecode(model, encoder_out, T_in, spkembs, need_attn, source is None, **kwargs)
        st.run(mode, model.TTS_POLL_STEPS, stats, profile=bool(getattr(model, "tts_profile", False)))
    if side != cur:
        cur.wait_stream(side)
    model.tts_polls = stats["polls"]
    model.tts_device_steps = stats["device_steps"]
    model.tts_graph_replays = stats["graph_replays"]
    model.tts_stats = stats
    steps = st.steps.tolist()
    if side != cur:
        for t in (st.mel_rec, st.prob_rec, st.rec):
            if t is not None:
                t.record_stream(cur)
    return st.mel_rec, st.prob_rec, st.rec, steps, T_in
