"""Streaming speech synthesis: generate_speech_stream / synthesize_stream.  A fixed set of `rows` decoder rows is stepped by ONE step
program (step_program.py), captured once and replayed until the stream ends; a row whose utterance has stopped is handed to the next
waiting utterance at a poll.  A step costs the same whether 1 or 32 of its rows are live (it streams every decoder weight once), so
keeping the rows occupied turns a call's B / max_b(steps_b) into the stream's B / mean_b(steps_b).

What makes this possible is that every position-dependent launch of the step reads ONE POSITION PER ROW (`pos` int32 [rows], steps
completed by the row's current occupant) where generate_speech_batch's step reads one counter: the self-attention K|V slot write
(st5_gemm_skinny_rows), the self-attention (st5_lm_decode_attn_rows), the cross-attention's record column (st5_decode_cross_attn_rows),
the positional row (st5_tts_pe_add_rows) and the step tail (st5_tts_step_tail_rows).  The captured graph never changes: an admission
rewrites only the DATA the graph reads (st5_tts_rows_admit and one K|V projection per layer into the row's slice), between two groups
of replays, when nothing of the step is in flight.

Row state changes only at a poll.  Order of work there, all on the one decode stream:
  1. the copy-out of every finished row's records (in front of anything that overwrites them: stream order);
  2. the upload of the next group's pre-net dropout seeds;
  3. the K|V projections and one admit launch for the rows handed to waiting utterances;
  4. the next group of TTS_POLL_STEPS steps; behind it the encoder work of the next waiting utterances, so that the device has it
     done by the time the host returns from the next poll's wait.
"""
import collections
import time

import torch

from . import functional as Fn
from . import hip
from .step_program import GRAPH_WARMUP_STEPS, StepProgram, append_layers, capture, decode_stream
from .tts_graph import unsupported_reason

STREAM_MODES = ("device", "graph")


# ---- the scheduling decision: host only ----
def assign_rows(free_rows, n_waiting):
    """Which free row takes which waiting request at a poll: the free rows in ascending order take the waiting requests in arrival
    order.  Returns [(row, k)], k the index into the waiting queue."""
    return list(zip(sorted(free_rows), range(n_waiting)))


def stream_schedule(lengths, rows, poll_steps, with_plan=False):
    """The stream for requests that take lengths[i] decode steps each (arrival order), on `rows` rows polled every `poll_steps`
    ticks: (total ticks, completion order as request indices).  Rows finished at the same poll complete in row order; the stream
    ends at the first poll with no running row and no waiting request.  with_plan: also [(request, row, admission tick)].  This is
    the loop of SynthesisStream with the device left out: assign_rows decides, a row admitted at tick t with n steps is found
    finished at the first poll at or behind tick t + n."""
    if rows < 1 or poll_steps < 1:
        raise ValueError(f"rows and poll_steps must be at least 1, got rows={rows}, poll_steps={poll_steps}")
    lengths = [max(1, int(n)) for n in lengths]      # (a row runs at least one step: the stop rule is tested behind a step)
    waiting = collections.deque(range(len(lengths)))
    occupant, ends = [None] * rows, [0] * rows
    tick, order, plan = 0, [], []
    while True:
        for b in range(rows):
            if occupant[b] is not None and ends[b] <= tick:
                order.append(occupant[b])
                occupant[b] = None
        for b, _ in assign_rows([b for b in range(rows) if occupant[b] is None], len(waiting)):
            occupant[b] = waiting.popleft()
            ends[b] = tick + lengths[occupant[b]]
            plan.append((occupant[b], b, tick))
        if all(o is None for o in occupant):
            break
        tick += poll_steps
    return (tick, order, plan) if with_plan else (tick, order)


def _is_text(src):
    return not src.is_floating_point()


class StreamDecode:
    """Every buffer of a stream and its one step program: `rows` rows over at most S encoder positions and `cap` steps each."""

    def __init__(self, model, rows, S, cap, threshold, need_attn, use_spk, poll_steps, device):
        r = model.reduction_factor
        dev, dtype = device, Fn.compute_dtype()
        post, pre, dec = model.speech_decoder_postnet, model.speech_decoder_prenet, model.decoder
        odim = post.odim
        C = model.args.decoder_embed_dim
        layers = list(dec.layers)
        H = layers[0].self_attn.num_heads
        hd = C // H
        B = rows
        self.rows, self.S, self.cap, self.r, self.odim, self.C, self.threshold = rows, S, cap, r, odim, C, threshold
        self.layers = layers
        prog = self.prog = StepProgram(dev, dtype, B)
        new, lin = prog.new, prog.lin
        i32 = dict(dtype=torch.int32, device=dev)
        self.state = torch.zeros(3, B, **i32)                     # pos | done | steps: one image for the poll
        self.pos, self.done, self.steps = self.state[0], self.state[1], self.state[2]
        self.done.fill_(1)                                        # every row idle until it is admitted
        self.minlen_d, self.maxlen_d = torch.zeros(B, **i32), torch.zeros(B, **i32)
        self.active, self.tick = torch.zeros(1, **i32), torch.zeros(1, **i32)
        self.mel_rec = torch.zeros(B, cap * r, odim, dtype=torch.float32, device=dev)
        self.prob_rec = torch.zeros(B, cap * r, dtype=torch.float32, device=dev)
        # cap + 1 record columns: a finished row that waits for its hand-over keeps stepping at pos = its step count <= cap, and the
        # column it then writes must never be one of its record's (0 .. steps - 1)
        self.rec = torch.zeros(B, len(layers), H, cap + 1, S, dtype=torch.float32, device=dev) if need_attn else None
        self.nxt = torch.zeros(B, odim, dtype=dtype, device=dev)
        self.host = torch.empty(3, B, dtype=torch.int32, pin_memory=True)
        self.desc_host = torch.zeros(B, 4, dtype=torch.int32, pin_memory=True)
        self.desc = torch.zeros(B, 4, **i32)
        self.event = torch.cuda.Event()
        anc = torch.arange(B, **i32).unsqueeze(1).expand(B, cap).contiguous()
        attn_ws = Fn.lm_decode_attn_ws(B, cap, H, hd, dev)

        # ---- pre-net: Tacotron pre-net (dropout always on, seeds per tick), Linear, positional row per row, speaker integration ----
        inl, spe = pre.decoder_prenet[0], pre.decoder_prenet[1]
        tac = inl[0]
        p_drop = float(tac.dropout_rate)
        self.n_seeds = n_seeds = len(tac.prenet) if p_drop > 0 else 0
        self.seed_slots = self.seed_table = self.seed_host = None
        if n_seeds:
            # row t % poll_steps of the table holds tick t's seeds; the tail of tick t - 1 moves them into the slots.  The host
            # refills the whole table at every poll (ticks g*P + 1 .. g*P + P in front of group g), tick 0's go into the slots here
            self.seed_slots = Fn.next_seeds(n_seeds).to(dev)
            self.seed_table = torch.zeros(poll_steps, n_seeds, dtype=torch.int64, device=dev)
            self.seed_host = torch.zeros(poll_steps, n_seeds, dtype=torch.int64, pin_memory=True)
        x = self.nxt
        for k, blk in enumerate(tac.prenet):
            seed = ((1 << 63) | (self.seed_slots.data_ptr() + 8 * k)) if n_seeds else 0
            x = lin(x, [blk[0].weight], [blk[0].bias], new(B, blk[0].weight.shape[0]), act=Fn.ACT_RELU, dropout_p=p_drop, seed=seed)
        x = lin(x, [inl[1].weight], [inl[1].bias], new(B, C))
        table = spe.pe(cap, dev)
        alpha = spe.alpha.detach()
        self.spk_dst = self.spk_stage = None
        if use_spk:
            lin_s = pre.spkembs_layer[0]
            cat = torch.zeros(B, lin_s.weight.shape[1], dtype=dtype, device=dev)
            self.spk_dst = cat[:, C:]
            self.spk_stage = torch.zeros(B, cat.shape[1] - C, dtype=dtype, device=dev)
            prog.add(lambda x=x: Fn.tts_pe_add_rows(x, table, alpha, self.pos, cat))
            x = lin(cat, [lin_s.weight], [lin_s.bias], new(B, C), act=Fn.ACT_RELU)
        else:
            y = new(B, C)
            prog.add(lambda x=x, y=y: Fn.tts_pe_add_rows(x, table, alpha, self.pos, y))
            x = y

        # ---- decoder layers: zero-filled cross-attention K|V (no excluded key ever holds non-finite bits), all keys valid in idle rows ----
        self.kpm = torch.zeros(B, S, dtype=torch.uint8, device=dev)
        cross_ws = Fn.decode_cross_attn_ws(B, S, H, hd, dev)
        self.slots = [torch.zeros(B, cap, 2 * C, dtype=dtype, device=dev) for _ in layers]
        self.kvp = [torch.zeros(B * S, 2 * C, dtype=dtype, device=dev) for _ in layers]
        recs = [self.rec[:, li] if self.rec is not None else None for li in range(len(layers))]

        def self_attn(q, slots, ctx, H, hd):
            Fn.lm_decode_attn_rows(q, slots, anc, self.pos, 1, cap, H, hd, ctx, attn_ws)

        def cross_attn(li, q, ctx):
            Fn.decode_cross_attn_rows(q, self.kvp[li], 0, S, H, hd, ctx, self.pos, cap + 1, kpm=self.kpm, rec=recs[li], ws=cross_ws)

        x = append_layers(prog, x, layers, self.slots, cap, self.pos, self_attn, cross_attn, dec.layer_norm, per_row=True)

        nf = post.feat_out.weight.shape[0] + post.prob_out.weight.shape[0]
        y = lin(x, [post.feat_out.weight, post.prob_out.weight], [post.feat_out.bias, post.prob_out.bias], new(B, nf, dt=torch.float32),
                out_f32=True)
        prog.add(lambda: Fn.tts_step_tail_rows(y, r, odim, self.minlen_d, self.maxlen_d, self.done, self.steps, self.pos, self.threshold,
                                               self.mel_rec, self.prob_rec, self.nxt, self.active, self.tick, self.seed_table,
                                               self.seed_slots))
        prog.finish()

    def upload_seeds(self):
        """In front of a group of P ticks g*P .. g*P + P - 1: the seeds of ticks g*P + 1 .. g*P + P, drawn in tick order, tick t's into
        row t % P (the last of them into row 0: the group's last tail moves it into the slots for the next group's first tick)."""
        if not self.n_seeds:
            return
        P = self.seed_host.shape[0]
        s = Fn.next_seeds(P * self.n_seeds).view(P, self.n_seeds)
        self.seed_host[1:] = s[:P - 1]
        self.seed_host[0] = s[P - 1]
        self.seed_table.copy_(self.seed_host, non_blocking=True)

    def admit(self, pairs):
        """pairs: [(row, request)]; the K|V projection of each request into its row's slice of every layer's buffer, then one launch
        that resets the rows' state.  Columns at and beyond T_b of a slice keep what was there and are excluded by kpm."""
        S, C = self.S, self.C
        for i, (b, q) in enumerate(pairs):
            for li, layer in enumerate(self.layers):
                ca = layer.encoder_attn
                Fn.linear_into(q["enc"], [ca.k_proj.weight, ca.v_proj.weight], [ca.k_proj.bias, ca.v_proj.bias],
                               hip.operand(self.kvp[li], 2 * C, off=b * S * 2 * C), 2 * C)
            self.desc_host[i, 0], self.desc_host[i, 1], self.desc_host[i, 2], self.desc_host[i, 3] = b, q["T"], q["minlen"], q["maxlen"]
            if self.spk_stage is not None:
                self.spk_stage[i].copy_(q["spk"])
        self.desc.copy_(self.desc_host, non_blocking=True)
        Fn.tts_rows_admit(self.desc, len(pairs), self.pos, self.done, self.steps, self.minlen_d, self.maxlen_d, self.nxt, self.kpm,
                          self.spk_stage, self.spk_dst)

    def poll(self):
        """pos | done | steps of every row after the steps enqueued so far (one host read)."""
        self.host.copy_(self.state, non_blocking=True)
        self.event.record()
        self.event.synchronize()
        return self.host


class SynthesisStream:
    """The loop.  advance() is one poll: it returns the rows that finished there, raw (key, mel record, probs, attn, request)."""

    def __init__(self, model, requests, rows, max_src_len, mode, need_attn, **kwargs):
        from .speecht5 import tts_row_limits
        self.model, self.requests, self.rows, self.S, self.mode, self.need_attn = model, iter(requests), rows, max_src_len, mode, need_attn
        self.kwargs = kwargs
        self.P = int(model.TTS_POLL_STEPS)
        r = model.reduction_factor
        self.threshold = tts_row_limits([max_src_len], r, True, **kwargs)[0]
        self.cap = max(tts_row_limits([max_src_len], r, text, **kwargs)[3] for text in (True, False))
        self.use_spk = hasattr(model.speech_decoder_prenet, "spkembs_layer")
        self.st, self.graph = None, None
        self.ready, self.exhausted, self.refused = collections.deque(), False, []
        self.occupant = [None] * rows
        self.stats = {"polls": 0, "device_steps": 0, "graph_replays": 0, "admitted": 0}
        self.inflight, self.finished = False, False
        self.profile = bool(getattr(model, "tts_profile", False))
        self.spans = []

    # ---- one utterance, encoded alone as generate_speech encodes it ----
    def _encode(self, key, src, spk):
        from .speecht5 import tts_row_limits
        model, text = self.model, _is_text(src)
        if src.dim() != 1:
            return f"request {key!r}: the source must be one utterance [n], got shape {tuple(src.shape)}"
        if text and src.numel() > self.S:
            return f"request {key!r} has {src.numel()} tokens, more than max_src_len={self.S}"
        if self.use_spk and spk is None:
            return f"request {key!r}: spkembs is required (spk_embed_integration_type 'pre')"
        if not self.use_spk and spk is not None:
            return f"request {key!r}: " + str(unsupported_reason(model, spk))
        if text:
            enc = model.forward_text_encoder(src.unsqueeze(0))
        else:
            enc = model.forward_encoder(src.unsqueeze(0), padding_mask=torch.zeros(1, src.numel(), dtype=torch.bool, device=src.device))
        enc = enc["encoder_out"][0]                                # [T, 1, C]
        T = int(enc.size(0))
        if T > self.S or T < 1:
            return f"request {key!r} has {T} encoder positions, outside 1 .. max_src_len={self.S}"
        _, minlen, maxlen, _ = tts_row_limits([T], model.reduction_factor, text, **self.kwargs)
        q = {"key": key, "T": T, "minlen": minlen[0], "maxlen": maxlen[0], "enc": Fn.as_compute(enc[:, 0].contiguous()), "spk": None}
        if spk is not None:
            q["spk"] = Fn.as_compute(torch.nn.functional.normalize(spk.float().view(1, -1)).contiguous()).view(-1)
        return q

    def _fill_ready(self):
        """Encoder work of the next waiting utterances, at most `rows` of them ahead of their admission."""
        while not self.exhausted and len(self.ready) < self.rows:
            try:
                key, src, spk = next(self.requests)
            except StopIteration:
                self.exhausted = True
                break
            q = self._encode(key, src, spk)
            if isinstance(q, str):
                self.refused.append(q)            # (the stream carries on with the next request; raised when it ends)
            else:
                self.ready.append(q)

    def _group(self):
        st, stats = self.st, self.stats
        n, e0 = 0, None

        def span(open_next):
            """profile: HIP events around the steps enqueued since the last call (the capture lies between two spans, as in run_steps)"""
            nonlocal n, e0
            if not self.profile:
                return
            if e0 is not None and n:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                self.spans.append((e0, e1, n))
            n, e0 = 0, None
            if open_next:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
        span(True)
        for _ in range(self.P):
            if self.mode == "graph" and stats["device_steps"] >= GRAPH_WARMUP_STEPS:
                if self.graph is None:
                    span(False)
                    t0 = time.perf_counter()
                    self.graph = capture(st.prog.step)
                    stats["capture_s"] = time.perf_counter() - t0
                    span(True)
                self.graph.replay()
                stats["graph_replays"] += 1
            else:
                st.prog.step()
                stats["device_steps"] += 1
                if self.mode == "graph":      # (the warm-up step in front of the capture is not a replay: not timed, as in run_steps)
                    n -= 1
            n += 1
        span(False)

    def advance(self):
        st, out = self.st, []
        if self.inflight:
            host = st.poll()
            self.stats["polls"] += 1
            self.inflight = False
            done, steps = host[1].tolist(), host[2].tolist()
            r = st.r
            for b in range(self.rows):                                       # 1. copy-out, in row order
                q = self.occupant[b]
                if q is None or not done[b]:
                    continue
                L = steps[b]
                attn = st.rec[b, :, :, :L, :q["T"]].contiguous() if st.rec is not None else None
                out.append((q["key"], st.mel_rec[b, :L * r].clone(), st.prob_rec[b, :L * r].clone(), attn))
                self.occupant[b] = None
        self._fill_ready()
        if st is None and self.ready:
            st = self.st = StreamDecode(self.model, self.rows, self.S, self.cap, self.threshold, self.need_attn, self.use_spk, self.P,
                                        self.ready[0]["enc"].device)
        free = [b for b in range(self.rows) if self.occupant[b] is None]
        pairs = [(b, self.ready[k]) for b, k in assign_rows(free, len(self.ready))]
        if not pairs and all(o is None for o in self.occupant):
            self.finished = True                                             # no running row, no waiting request
            return out
        st.upload_seeds()                                                    # 2.
        if pairs:                                                            # 3.
            st.admit(pairs)
            for b, q in pairs:
                self.occupant[b] = self.ready.popleft()
                assert self.occupant[b] is q
            self.stats["admitted"] += len(pairs)
        self._group()                                                        # 4.
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
        m = self.model
        m.tts_polls, m.tts_device_steps, m.tts_graph_replays = self.stats["polls"], self.stats["device_steps"], self.stats["graph_replays"]
        m.tts_decode_mode, m.tts_stats = self.mode, self.stats


def check_arguments(model, rows, max_src_len, decode):
    """The refusals that need no request: a ValueError naming the argument, before anything is enqueued."""
    if decode not in STREAM_MODES:
        raise ValueError(f"decode must be one of {STREAM_MODES} for a stream (the eager loop has a host step index), got {decode!r}")
    if not isinstance(rows, int) or rows < 1:
        raise ValueError(f"rows must be an integer >= 1, got {rows!r}")
    if not isinstance(max_src_len, int) or max_src_len < 1:
        raise ValueError(f"max_src_len must be an integer >= 1, got {max_src_len!r}")
    why = unsupported_reason(model, None)
    if why is not None:
        raise ValueError(f"model: generate_speech_stream is not available: {why}")


def run_stream(model, requests, rows, max_src_len, decode, need_attn, finish, **kwargs):
    """The generator behind generate_speech_stream / synthesize_stream.  finish(list of raw (key, mel record [L*r, odim], probs,
    attn)) turns the rows that completed at one poll into what is yielded for them.  The decode stream (step_program.decode_stream
    for "graph") is entered for each poll and left before anything is yielded, so the consumer runs on its own stream between two polls.  The argument checks run at the
    call, not at the first next()."""
    check_arguments(model, rows, max_src_len, decode)
    return _run(model, requests, rows, max_src_len, decode, need_attn, finish, **kwargs)


def _run(model, requests, rows, max_src_len, decode, need_attn, finish, **kwargs):
    stream = SynthesisStream(model, requests, rows, max_src_len, decode, need_attn, **kwargs)
    device = next(model.parameters()).device
    # The two streams are ordered only where something crosses between them: the consumer's stream in front of the decode stream at
    # the start and behind every poll that yielded (the consumer ran: its next requests may come from its stream), the decode stream
    # in front of the consumer's at every poll that yields.  Ordering them at every poll put ~1.2 ms of cross-stream waiting in
    # front of each group of replays (0.15 ms per step at 8 steps per poll; profiles/tts_stream_timing.json).  The request
    # iterator is advanced inside the decode stream's context, so what it creates is created there.
    order_in, side = True, None
    try:
        while not stream.finished:
            cur = torch.cuda.current_stream(device)
            side = decode_stream(model, device) if decode == "graph" else cur
            if side != cur and order_in:
                side.wait_stream(cur)
            order_in = False
            with torch.no_grad(), torch.cuda.stream(side):
                results = finish(stream.advance())
            if results and side != cur:
                for item in results:
                    for t in item:
                        if isinstance(t, torch.Tensor):
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
    if stream.refused:
        raise ValueError("requests: refused " + "; ".join(stream.refused))
