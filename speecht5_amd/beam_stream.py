"""Streaming ASR / ST beam search: SequenceGenerator.generate_stream.  A fixed set of `sentences` slots of `beam` hypothesis rows each
is stepped by ONE step program (step_program.py), enqueued kernel by kernel ("device") or captured once and replayed until the stream
ends ("graph"); a slot whose sentence has finished is handed to the next waiting request at a poll.  generate(decode="device" /
"graph") keeps every sentence of a call in the batch until the last one has finished (beam_graph.py), so a call costs max(steps) per
sentence; the stream costs mean(steps), as the synthesis stream does for TTS (tts_stream.py).  Attention-only search (the ST recipe
and ASR decoding without CTC) by default; joint CTC / attention scoring with generate_stream(joint_ctc=True) and Transformer-LM
shallow fusion for a generator built with an lm_model, alone or together (the ASR recipe), see below.

What makes it possible is that every position-dependent launch of the step reads the position of the SLOT where beam_graph's step
reads one counter: the pre-net row (st5_beam_embed_sents), the self-attention K|V slot write (st5_gemm_skinny_rows over pos_rows), the
self-attention (st5_lm_decode_attn_rows), the beam step (st5_beam_step_sents: step = pos[s], max_len = maxlen[s] per workgroup) and
the ancestry reorder (st5_beam_reorder_sents).  st5_beam_cross_attn has no step dependence and is launched as it is.  There is no
global counter, no arrival ticket and no finished-sentence count: a slot's position is read and written by its own workgroup only,
so the hand-off between two launches is the kernel boundary.  A slot that is done (finished or idle) costs what a live one costs in
every launch but the beam step and the reorder, which return at once for it: the GEMMs stream every weight once whatever the rows.

The captured graph never changes.  An admission rewrites only the DATA the graph reads, between two groups of steps, when nothing of
the step is in flight: one st5_beam_sents_admit launch (the slot's beam-step state, its record header, its key-padding bytes), the
K|V projection of the sentence's encoder rows into the slot's slice of every layer's encoder-side buffer, and a zero fill of the
slice behind the sentence's frames.  The projection runs in the shape it has in a generate() call on that sentence alone (its own
frames as rows, all layers in one GEMM), so the K|V bits are that call's.

Order of work at a poll, all on the one decode stream:
  1. the records of finished sentences are copied out (in stream order, in front of anything that overwrites them);
  2. the finished slots are handed to waiting requests (tts_stream.assign_rows): projections, zero fills, one admit launch;
  3. the next group of BEAM_POLL_STEPS steps; behind it the encoder work of the next waiting requests.

A result does not depend on the slot, the admission tick or the neighbours: hypothesis rows never read another slot's rows (the
GEMMs, the LayerNorms and the attentions are per row or per sentence, the beam step per sentence), and it is bit-equal to
generate(decode="graph", exact_rows=True) on the sentence alone as long as the cross-attention's key split, a function of S alone
(csrc/beam_decode.hip), is the same: up to 64 encoder positions per slot there is one range whatever S is.

Joint CTC / attention scoring (joint_ctc=True; ctc_weight > 0 with ctc_rows=True): the step program becomes beam_graph.py's CTC step
with every launch in its per-slot form: pre-net row, layers, projection, st5_beam_ctc_candidates_sents, st5_ctc_prefix_score_rows_sents,
st5_beam_step_sents_logprobs on the mixed log-probabilities, st5_ctc_select_sents, st5_beam_reorder_sents (csrc/beam_ctc.hip; buffers:
functional.BeamCtcStreamState).  Slot s has its own slice of the posterior x [n_slots, S, V], its own frame count frames[s] and its own
rows of every CTC buffer; no kernel reads another slot's.  A request's posterior is the log-softmax of the CTC projection of ITS OWN
encoder call (_encode: forward_encoder(exact_rows=True) on the sentence alone, T rows through the projection's GEMM), which is the call
shape of generate(exact_rows=True) on that sentence alone, padded or not: forward_encoder_rows strips a row's padding before the
encoder, so the single call's projection has the same T rows and BeamDeviceDecode._ctc_state sees the same bits.  An admission copies
the posterior into the slot's slice and launches st5_ctc_sents_admit behind st5_beam_sents_admit (frames, the initial prefix states,
prev = 0, unknown = 0).  Without joint_ctc the launch list is what it is without this paragraph.

Joint scoring brings a per-sentence failure: a hypothesis continued by a token outside its CTC candidates has no prefix state
(_generate raises KeyError for the call).  Here the flag is per slot (`unknown` [n_slots]), read at every poll beside the state image.
A flagged slot yields nothing, finished or not: its key goes to stream.failed and beam_stream_stats["failed"], its occupant is cleared
and the slot is handed on like a finished one (the admission clears the flag; if nobody waits the slot runs on to its limit and is
never read).  When the stream ends the failed keys are raised in one KeyError (with the refusals' text when there are any); every other
sentence has completed by then.

Shallow fusion (a generator built with lm_model; no keyword: such a generator was refused before): the LM's step in its per-slot form
(TransformerLanguageModel.device_step_sents: st5_beam_embed_sents with the LM's tables, the layers with K|V into slot pos_rows[r],
st5_lm_decode_attn_rows, the final LayerNorm, the output projection with fp32 output) follows the decoder's projection, then
st5_beam_lm_logprobs_sents (csrc/beam_lm.hip) puts the LM term into the step's log-probabilities, in beam_graph.py's order.  Without
CTC: st5_beam_lm_logprobs_sents on the decoder's logits into lp [rows, V], st5_beam_step_sents_logprobs on lp, the reorder.  With
joint_ctc: candidates, prefix scores and mix, st5_beam_lm_logprobs_sents in place on ctc.lp, st5_beam_step_sents_logprobs, select, the
reorder.  The LM's slot caches are read through the stream's ONE ancestry table (init_decode(anc=bs.anc)), which the admission resets
and the reorder reorders; an admission does nothing for the LM, and a handed-over slot's stale K|V are never read (device_step_sents
says why).  Refused, each with a ValueError naming lm_model before anything is enqueued: an LM that is not a TransformerLanguageModel,
V_lm > vocab_size, and cap + 2 positions more than lm.max_positions() (cap: the step limit at max_src_len, which every request's limit
is held to).  Without an LM the launch list is what it is without this paragraph."""
import collections
import time

import torch

from . import functional as Fn
from . import beam_graph
from .step_program import GRAPH_WARMUP_STEPS, StepProgram, append_layers, capture, decode_stream
from .tts_stream import assign_rows

STREAM_MODES = ("device", "graph")
MAX_ROWS = Fn.SKINNY_MAX_M      # sentences * beam: one launch of the skinny-M GEMM


def step_limit(gen, src_len, max_len=None):
    """The step limit of a request of src_len samples: generate()'s formula on its own length, or the request's max_len."""
    return int(max_len) if max_len is not None else min(int(gen.max_len_a * src_len + gen.max_len_b), gen.max_len - 1)


def check_arguments(gen, sentences, max_src_len, decode, joint_ctc=False):
    """The refusals that need no request: a ValueError naming the option, before anything is enqueued."""
    if decode not in STREAM_MODES:
        raise ValueError(f"decode must be one of {STREAM_MODES} for a stream (the other loops have a host step index), got {decode!r}")
    if joint_ctc:
        if not gen.ctc_weight > 0:
            raise ValueError(f"generate_stream: joint_ctc=True needs a generator with ctc_weight > 0, got ctc_weight={gen.ctc_weight}")
        if not gen.ctc_rows:
            raise ValueError("generate_stream: joint_ctc=True needs ctc_rows=True (every slot is scored against its own sentence's CTC "
                             "posterior; the first-sentence scoring of ctc_rows=False is decode='slots' only)")
        enc = getattr(gen.model.models[0], "encoder", None)
        if getattr(enc, "proj", None) is None:
            raise ValueError("generate_stream: joint_ctc=True needs a model whose encoder has a CTC projection")
    elif gen.ctc_weight > 0:
        raise ValueError("generate_stream: ctc_weight > 0 needs joint_ctc=True (joint CTC / attention scoring per sentence slot; a "
                         "sentence whose hypothesis leaves its CTC candidates then fails by key, see generate_stream) or generate()")
    if gen.lm_model is not None:
        # in front of check_generator, which refuses the same LMs in the words of generate()'s `decode` modes
        from .transformer_lm import TransformerLanguageModel
        if not isinstance(gen.lm_model, TransformerLanguageModel):
            raise ValueError(f"generate_stream: an LM (lm_model) of type {type(gen.lm_model).__name__} is not supported (only "
                             f"speecht5_amd.transformer_lm.TransformerLanguageModel has a per-sentence step); use generate()")
        V_lm = gen.lm_model.decoder.output_projection.weight.shape[0]      # the columns of the LM's logits, what the kernel is given
        if V_lm > gen.vocab_size:
            raise ValueError(f"generate_stream: lm_model has a dictionary of {V_lm} symbols, more than the model's {gen.vocab_size}")
    beam_graph.check_generator(gen)
    if not isinstance(sentences, int) or isinstance(sentences, bool) or sentences < 1:
        raise ValueError(f"sentences must be an integer >= 1, got {sentences!r}")
    if sentences * gen.beam_size > MAX_ROWS:
        raise ValueError(f"sentences={sentences} x beam_size={gen.beam_size} is more than {MAX_ROWS} hypothesis rows (one skinny-M GEMM launch)")
    if not isinstance(max_src_len, int) or isinstance(max_src_len, bool) or max_src_len < 1:
        raise ValueError(f"max_src_len must be an integer >= 1 (samples), got {max_src_len!r}")
    model = gen.model.models[0]
    if not hasattr(model, "speech_encoder_prenet"):
        raise ValueError(f"generate_stream needs a speech encoder pre-net; {type(model).__name__} has none")
    S = int(model.speech_encoder_prenet._frames(max_src_len))
    if S < 1:
        raise ValueError(f"max_src_len={max_src_len} samples give no encoder position")
    cap = step_limit(gen, max_src_len)
    if cap < gen.min_len:
        raise ValueError(f"max_src_len={max_src_len}: the step limit {cap} is below min_len={gen.min_len}")
    if gen.lm_model is not None and cap + 2 > gen.lm_model.max_positions():
        # every request's limit is held to cap (BeamStream._encode), so this covers them all
        raise ValueError(f"generate_stream: lm_model takes {gen.lm_model.max_positions()} positions, the step limit at max_src_len="
                         f"{max_src_len} needs cap + 2 = {cap + 2}; lower max_src_len, max_len_a or max_len_b")
    return S, cap


class BeamStreamDecode:
    """Every buffer of a stream and its one step program: n_slots slots x beam rows over at most S encoder positions and step limits
    up to `cap`.  It outlives the graph that has its buffers baked in."""

    def __init__(self, gen, model, n_slots, S, cap, device, joint_ctc=False):
        beam, V = gen.beam_size, gen.vocab_size
        dec, pre, post = model.decoder, model.text_decoder_prenet, model.text_decoder_postnet
        dev, dtype = device, Fn.compute_dtype()
        layers = self.layers = list(dec.layers)
        sa, ca = layers[0].self_attn, layers[0].encoder_attn
        H, hd, C = sa.num_heads, sa.head_dim, sa.embed_dim
        rows, Tmax = n_slots * beam, cap + 2
        self.gen, self.n_slots, self.beam, self.S, self.cap, self.C, self.rows = gen, n_slots, beam, S, cap, C, rows
        i32 = dict(dtype=torch.int32, device=dev)
        anc = torch.arange(rows, **i32).unsqueeze(1).expand(rows, Tmax).contiguous()
        bs = self.bs = Fn.BeamStreamState(n_slots, beam, cap, dev, anc=anc)
        self.never = beam_graph.never_mask(gen, dev)
        self.len_div = Fn.beam_len_div(cap, gen.len_penalty, dev) if gen.normalize_scores else None
        self.host = torch.zeros(bs.image.numel(), dtype=torch.int32, pin_memory=True)
        self.desc_host = torch.zeros(n_slots, 4, dtype=torch.int32, pin_memory=True)
        self.desc = torch.zeros(n_slots, 4, **i32)
        self.event = torch.cuda.Event()
        self.ctc = self.unknown_host = None
        if joint_ctc:                               # (nc as BeamDeviceDecode._ctc_state computes it)
            from .sequence_generator import CTC_SCORING_RATIO
            V_ctc = model.encoder.proj.weight.shape[0]
            nc = self.ctc_beam = min(V_ctc - gen.mask_idxs.numel(), int(beam * CTC_SCORING_RATIO))
            self.ctc = Fn.BeamCtcStreamState(bs, S, V_ctc, nc, gen.ctc_weight, gen.blank, gen.eos, dev)
            self.unknown_host = torch.zeros(n_slots, dtype=torch.int32, pin_memory=True)
        # self-attention slot caches and the encoder side once per slot, zero-filled: no excluded key and no idle row ever holds
        # non-finite bits; all keys valid in idle slots
        self.kv = [torch.zeros(rows, Tmax, 2 * C, dtype=dtype, device=dev) for _ in layers]
        self_ws = Fn.lm_decode_attn_ws(rows, Tmax, H, hd, dev)
        self.kpm = torch.zeros(n_slots, S, dtype=torch.uint8, device=dev)
        cross = [l.encoder_attn for l in layers]
        ws_ = [w for a in cross for w in (a.k_proj.weight, a.v_proj.weight)]
        bs_ = [b for a in cross for b in (a.k_proj.bias, a.v_proj.bias)]
        # the projections as TransformerDecoder.init_beam_slots groups them: all layers in one GEMM where their shapes allow it
        if all(b is not None for b in bs_) and all(w.shape == ws_[0].shape for w in ws_):
            kv_all = torch.zeros(n_slots * S, len(cross) * 2 * C, dtype=dtype, device=dev)
            self.xkv = [(kv_all, idx * 2 * C) for idx in range(len(cross))]
            self.proj = [(ws_, bs_, kv_all)]
        else:
            self.xkv = [(torch.zeros(n_slots * S, 2 * C, dtype=dtype, device=dev), 0) for _ in cross]
            self.proj = [([a.k_proj.weight, a.v_proj.weight], [a.k_proj.bias, a.v_proj.bias], kv) for a, (kv, _) in zip(cross, self.xkv)]
        cross_ws = Fn.beam_cross_attn_ws(rows, S, ca.num_heads, ca.head_dim, dev)
        sent = torch.arange(n_slots, **i32)

        prog = self.prog = StepProgram(dev, dtype, rows)
        new, lin, add = prog.new, prog.lin, prog.add
        # pre-net: embed_scale * E[token] + pos[pos[slot] + padding_idx + 1] (beam_graph.py: the step decides the position)
        table = pre.embed_tokens.weight.detach()
        pos = pre.embed_positions.table(cap + 2 + pre.padding_idx + 2, dev)
        x = new(rows, C)
        add(lambda x=x: Fn.beam_embed_sents(table, bs, pos, pre.padding_idx + 1, pre.embed_scale, x))

        def self_attn(q, slots, ctx, H, hd):      # positions 0 .. pos[slot] over the one ancestry table, reordered in place
            Fn.lm_decode_attn_rows(q, slots, bs.anc, bs.pos_rows, 1, Tmax, H, hd, ctx, self_ws)

        def cross_attn(idx, q, ctx):              # no step dependence
            a, (kv, k_off) = layers[idx].encoder_attn, self.xkv[idx]
            Fn.beam_cross_attn(q, kv, k_off, sent, n_slots, beam, S, a.num_heads, a.head_dim, kpm=self.kpm, ws=cross_ws, ctx=ctx)

        x = append_layers(prog, x, layers, self.kv, Tmax, bs.pos_rows, self_attn, cross_attn, dec.layer_norm, per_row=True)
        proj = post.output_projection
        self.logits = lin(x, [proj.weight], [proj.bias], new(rows, V, dt=torch.float32), out_f32=True)
        rules = dict(temperature=gen.temperature, pad=gen.pad, unk=gen.unk, eos=gen.eos, unk_penalty=gen.unk_penalty, min_len=gen.min_len)
        # shallow fusion: the LM's per-row step over the same rows and the stream's one ancestry table, behind the decoder's projection
        # (beam_graph.py's order).  Its caches and lp need no fill: a row's attention reads positions 0 .. pos_rows[r] of its own slot,
        # all written by the occupant's steps (an idle slot stands at position 0 and rewrites it in every step), and a slot that is
        # done or idle never has its LM logits or its rows of lp read (st5_beam_lm_logprobs_sents and the beam step return for it).
        lm, w_lm = gen.lm_model, float(gen.lm_weight)
        self.lm_state = self.lm_logits = self.lp = None
        if lm is not None:
            self.lm_state = lm.init_decode(rows, Tmax, anc=bs.anc)
            self.lm_logits = lm.device_step_sents(self.lm_state, bs, prog)
        if self.ctc is None and lm is None:
            add(lambda: Fn.beam_step_sents(self.logits, V, bs, self.never, self.len_div, **rules))
        elif self.ctc is None:
            # log-probabilities with the LM term, the beam step on them
            self.lp = new(rows, V, dt=torch.float32)
            add(lambda: Fn.beam_lm_logprobs_sents(self.lp, V, bs, self.lm_logits, w_lm, logits=self.logits, temperature=gen.temperature))
            add(lambda: Fn.beam_step_sents_logprobs(self.lp, V, bs, self.never, self.len_div, **rules))
        else:
            # beam_graph.py's CTC step per slot: log-probabilities and candidates, prefix scores mixed into them, [the LM term,] the
            # beam step on them, the continued rows' prefix states
            ctc = self.ctc
            add(lambda: Fn.beam_ctc_candidates_sents(self.logits, V, bs, ctc, self.never, gen.temperature))
            add(lambda: Fn.ctc_prefix_score_rows_sents(bs, ctc))
            if lm is not None:
                add(lambda: Fn.beam_lm_logprobs_sents(ctc.lp, V, bs, self.lm_logits, w_lm))
            add(lambda: Fn.beam_step_sents_logprobs(ctc.lp, V, bs, self.never, self.len_div, **rules))
            add(lambda: Fn.ctc_select_sents(bs, ctc))
        add(lambda: Fn.beam_reorder_sents(bs))
        prog.finish()

    def buffer_ptrs(self):
        """Data pointers of what the graph has baked in and must never move: slot K/V, encoder-side K|V, key-padding bytes, the
        beam-step state, its image and the records; with joint_ctc the CTC buffers; with an LM its slot caches, its logits and
        (without CTC) the fused log-probabilities."""
        bs = self.bs
        ctc = () if self.ctc is None else tuple(t.data_ptr() for t in self.ctc.buffers())
        lm = () if self.lm_state is None else tuple(t.data_ptr() for t in self.lm_state.kv) + tuple(
            t.data_ptr() for t in (self.lm_logits, self.lp) if t is not None)
        return tuple(t.data_ptr() for t in self.kv) + tuple(kv.data_ptr() for kv, _ in self.xkv) + tuple(
            t.data_ptr() for t in (self.kpm, bs.anc, bs.tok, bs.score, bs.image, bs.pos_rows, bs.rec_tok, bs.rec_pos, self.logits)) + ctc + lm

    def admit(self, pairs, bos):
        """pairs: [(slot, request)].  Per request the K|V projection of its encoder rows (the single call's GEMM shape) into the slot's
        slice of the encoder-side buffers and a zero fill behind its frames; then one launch that resets the slots' state.  With
        joint_ctc the request's CTC posterior goes into the slot's slice of ctc.x and a second launch resets the slots' CTC state."""
        S = self.S
        for i, (s, q) in enumerate(pairs):
            T = q["T"]
            for weights, biases, dst in self.proj:
                dst[s * S:s * S + T].copy_(Fn.linear(q["enc"], weights, biases))
                if T < S:
                    dst[s * S + T:(s + 1) * S].zero_()
            if self.ctc is not None:
                self.ctc.x[s, :T].copy_(q["post"])
            self.desc_host[i, 0], self.desc_host[i, 1], self.desc_host[i, 2], self.desc_host[i, 3] = s, q["max_len"], T, bos
        self.desc.copy_(self.desc_host, non_blocking=True)
        Fn.beam_sents_admit(self.desc, len(pairs), self.bs, self.kpm)
        if self.ctc is not None:
            Fn.ctc_sents_admit(self.desc, len(pairs), self.bs, self.ctc)

    def poll(self):
        """The state image after the steps enqueued so far (one pinned non-blocking copy and an event): pos, maxlen, done, moved,
        n_hyp, rec_len, rec_score as host views, and the CTC scorer's per-slot `unknown` flags (None without joint_ctc), read where the
        image is read."""
        self.host.copy_(self.bs.image, non_blocking=True)
        if self.ctc is not None:
            self.unknown_host.copy_(self.ctc.unknown, non_blocking=True)
        self.event.record()
        self.event.synchronize()
        return self.bs.unpack_image(self.host) + (self.unknown_host,)

    def copy_out(self, s):
        """Device copies of slot s's records, enqueued in front of whatever overwrites them."""
        b0, b1 = s * self.beam, (s + 1) * self.beam
        bs = self.bs
        return bs.rec_tok[b0:b1].clone(), bs.rec_pos[b0:b1].clone(), bs.rec_score[b0:b1].clone()


class BeamStream:
    """The loop.  advance() is one poll: it returns [(key, hyps)] of the sentences found finished there, in slot order."""

    def __init__(self, gen, requests, sentences, max_src_len, S, cap, mode, joint_ctc=False):
        self.gen, self.model, self.requests = gen, gen.model.models[0], iter(requests)
        self.n_slots, self.max_src_len, self.S, self.cap, self.mode = sentences, max_src_len, S, cap, mode
        self.joint_ctc, self.failed = bool(joint_ctc), []
        self.P = int(gen.BEAM_POLL_STEPS)
        self.st, self.graph = None, None
        self.ready, self.exhausted, self.refused = collections.deque(), False, []
        self.occupant = [None] * sentences
        self.stats = {"polls": 0, "device_steps": 0, "graph_replays": 0, "admitted": 0, "sentence_steps": {}}
        if self.joint_ctc:
            self.stats["failed"] = []
        self.inflight, self.finished = False, False
        self.first_ptrs = None
        self.profile = bool(getattr(gen, "beam_profile", False))
        self.spans = []

    # ---- one request, encoded alone as generate(exact_rows=True) encodes a row ----
    def _encode(self, req):
        gen = self.gen
        if not isinstance(req, (tuple, list)) or len(req) not in (2, 3):
            return f"request {req!r}: expected (key, source) or (key, source, max_len)"
        key, src = req[0], req[1]
        max_len = req[2] if len(req) == 3 else None
        if not isinstance(src, torch.Tensor) or not src.is_floating_point():
            return (f"request {key!r}: the source must be an fp32 waveform [n] (text sources have no stream), got "
                    f"{getattr(src, 'dtype', type(src).__name__)}")
        if src.dim() != 1 or src.numel() < 1:
            return f"request {key!r}: the source must be one waveform [n], got shape {tuple(src.shape)}"
        n = int(src.numel())
        if n > self.max_src_len:
            return f"request {key!r} has {n} samples, more than max_src_len={self.max_src_len}"
        limit = step_limit(gen, n, max_len)
        if limit > self.cap:
            return f"request {key!r}: max_len {limit} is above the stream's cap {self.cap} (the step limit at max_src_len)"
        if limit < gen.min_len:
            return f"request {key!r}: max_len {limit} is below min_len={gen.min_len}"
        net_input = {"source": src.unsqueeze(0), "padding_mask": torch.zeros(1, n, dtype=torch.bool, device=src.device)}
        out = gen.model.forward_encoder(net_input, exact_rows=True)[0]
        enc = out["encoder_out"][0]                                                               # [T, 1, C]
        T = int(enc.size(0))
        if T > self.S or T < 1:
            return f"request {key!r} has {T} encoder positions, outside 1 .. {self.S} (max_src_len={self.max_src_len})"
        q = {"key": key, "T": T, "max_len": limit, "enc": Fn.as_compute(enc[:, 0].contiguous())}
        if self.joint_ctc:
            # the posterior [T, V] as BeamDeviceDecode._ctc_state builds it in a call on this sentence alone (module docstring)
            post = self.model.get_normalized_probs_for_ctc(out, log_probs=True).transpose(0, 1)   # 1 x T x V
            q["post"] = post.detach().float().contiguous()[0]
        return q

    def _fill_ready(self):
        """Encoder work of the next waiting requests, at most `sentences` of them ahead of their admission."""
        while not self.exhausted and len(self.ready) < self.n_slots:
            try:
                req = next(self.requests)
            except StopIteration:
                self.exhausted = True
                break
            q = self._encode(req)
            if isinstance(q, str):
                self.refused.append(q)            # (the stream carries on with the next request; raised when it ends)
            else:
                self.ready.append(q)

    def _group(self):
        st, stats = self.st, self.stats
        e0 = None
        n = 0
        for _ in range(self.P):
            if self.mode == "graph" and stats["device_steps"] >= GRAPH_WARMUP_STEPS:
                if self.graph is None:
                    t0 = time.perf_counter()
                    self.graph = capture(st.prog.step)
                    stats["capture_s"] = time.perf_counter() - t0
                if self.profile and e0 is None:
                    e0 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                self.graph.replay()
                stats["graph_replays"] += 1
                n += 1
            else:
                if self.profile and self.mode != "graph" and e0 is None:
                    e0 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                st.prog.step()
                stats["device_steps"] += 1
                n += self.mode != "graph"         # (the warm-up step in front of the capture is not timed, as in run_steps)
        if e0 is not None and n:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.spans.append((e0, e1, n))

    def _hyps(self, raw, n_hyp, lengths, scores):
        """generate()'s hypotheses of one sentence from its copied-out records: best first, by BeamDeviceDecode.finalized's sort."""
        rec_tok, rec_pos, rec_score = raw
        hyps = []
        for k in range(n_hyp):
            n = int(lengths[k])
            hyps.append({"tokens": rec_tok[k, :n].to(torch.int64), "score": rec_score[k].clone(), "attention": torch.empty(0),
                         "alignment": torch.empty(0), "positional_scores": rec_pos[k, :n].clone()})
        order = torch.sort(scores[:n_hyp], descending=True)[1]
        return [hyps[i] for i in order]

    def advance(self):
        st, out = self.st, []
        if self.inflight:
            pos, _, done, _, n_hyp, rec_len, rec_score, unknown = st.poll()
            self.stats["polls"] += 1
            self.inflight = False
            beam = st.beam
            for s in range(self.n_slots):                                    # 1. copy-out, in slot order
                q = self.occupant[s]
                if q is None:
                    continue
                if unknown is not None and int(unknown[s]):
                    # a hypothesis left its CTC candidates: the sentence fails, finished or not, and its slot is handed on
                    self.failed.append(q["key"])
                    self.stats["failed"].append(q["key"])
                    self.occupant[s] = None
                    continue
                if not int(done[s]):
                    continue
                b0 = s * beam
                out.append((q["key"], self._hyps(st.copy_out(s), int(n_hyp[s]), rec_len[b0:b0 + beam].clone(),
                                                 rec_score[b0:b0 + beam].clone())))
                self.stats["sentence_steps"][q["key"]] = int(pos[s])
                self.occupant[s] = None
        self._fill_ready()
        if st is None and self.ready:
            st = self.st = BeamStreamDecode(self.gen, self.model, self.n_slots, self.S, self.cap, self.ready[0]["enc"].device,
                                            joint_ctc=self.joint_ctc)
            self.first_ptrs = st.buffer_ptrs()
        free = [s for s in range(self.n_slots) if self.occupant[s] is None]
        pairs = [(s, self.ready[k]) for s, k in assign_rows(free, len(self.ready))]
        if not pairs and all(o is None for o in self.occupant):
            self.finished = True                                             # no running slot, no waiting request
            return out
        if pairs:                                                            # 2.
            st.admit(pairs, self.gen.eos)
            for s, q in pairs:
                self.occupant[s] = self.ready.popleft()
                assert self.occupant[s] is q
            self.stats["admitted"] += len(pairs)
        self._group()                                                        # 3.
        self.inflight = True
        self._fill_ready()                                                   # encode ahead, behind the group
        return out

    def close(self):
        if self.graph is not None:
            # released with nothing in flight: a CUDAGraph must never be destroyed inside a later capture
            torch.cuda.current_stream().synchronize()
            self.graph.reset()
            self.graph = None
        if self.profile and self.spans:
            torch.cuda.current_stream().synchronize()
            self.stats["step_ms"] = sum(a.elapsed_time(b) for a, b, _ in self.spans)
            self.stats["steps_timed"] = sum(n for _, _, n in self.spans)
        g, stats = self.gen, self.stats
        g.beam_decode_mode = self.mode
        g.beam_polls, g.beam_device_steps, g.beam_graph_replays = stats["polls"], stats["device_steps"], stats["graph_replays"]
        g.beam_stream_stats = stats
        if self.st is not None:
            g.beam_buffer_ptrs = (self.first_ptrs, self.st.buffer_ptrs())


def run_stream(gen, requests, sentences, max_src_len, decode, joint_ctc=False):
    """The generator behind SequenceGenerator.generate_stream.  The argument checks run at the call, not at the first next().  The
    decode stream (step_program.decode_stream for "graph") is entered for each poll and left before anything is yielded, so the
    consumer runs on its own stream between two polls."""
    S, cap = check_arguments(gen, sentences, max_src_len, decode, joint_ctc)
    return _run(gen, requests, sentences, max_src_len, S, cap, decode, joint_ctc)


def _tensors(results):
    for _, hyps in results:
        for h in hyps:
            for t in (h["tokens"], h["score"], h["positional_scores"]):
                yield t


def _run(gen, requests, sentences, max_src_len, S, cap, decode, joint_ctc=False):
    stream = BeamStream(gen, requests, sentences, max_src_len, S, cap, decode, joint_ctc)
    model = gen.model.models[0]
    device = next(model.parameters()).device
    # The two streams are ordered only where something crosses between them (tts_stream._run): the consumer's stream in front of the
    # decode stream at the start and behind every poll that yielded, the decode stream in front of the consumer's at every poll that
    # yields.  The request iterator is advanced inside the decode stream's context, so what it creates is created there.
    order_in, side = True, None
    try:
        while not stream.finished:
            cur = torch.cuda.current_stream(device)
            side = decode_stream(model, device) if decode == "graph" else cur
            if side != cur and order_in:
                side.wait_stream(cur)
            order_in = False
            with torch.no_grad(), torch.cuda.stream(side):
                results = stream.advance()
            if results and side != cur:
                for t in _tensors(results):
                    t.record_stream(cur)
                cur.wait_stream(side)
                order_in = True
            yield from results
    finally:
        cur = torch.cuda.current_stream(device)
        with torch.cuda.stream(side if side is not None else cur):
            stream.close()
        if side is not None and side != cur:
            cur.wait_stream(side)
    refused = "requests: refused " + "; ".join(stream.refused) if stream.refused else ""
    if stream.failed:
        # _generate's KeyError, by key: the other sentences have completed
        raise KeyError(f"sentences {stream.failed!r}: a hypothesis was extended by a token outside its CTC candidate list "
                       f"(ctc_beam={stream.st.ctc_beam}); its prefix state does not exist" + ("; " + refused if refused else ""))
    if refused:
        raise ValueError(refused)
