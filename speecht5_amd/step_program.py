"""The mechanism of the device-stepped decode loops: batched TTS (tts_graph.py) and ASR beam search (beam_graph.py).

One decode step is a fixed sequence of kernel launches on caller-owned buffers (StepProgram): every GEMM of the step runs on the
weight-streaming skinny-M kernel (csrc/decode_gemm.hip), the self-attention K|V projection writes slot `counter` of a per-layer cache
through that kernel's device-side output offset (append_layers), and every launch that depends on the position reads ONE int32
counter in device memory (steps completed so far), which the step's last task-specific kernel advances.  Nothing in the step depends
on a host value, allocates, or builds a weight image, so the same sequence is enqueued kernel by kernel ("device": the warm-up and
debugging form) or captured once and replayed ("graph") by run_steps, which polls the host where replay_schedule says.

The captured step has no forked stream and no parallel branch: every launch goes to the one capturing stream.  No library entry
with a per-stream table is part of a step (st5_gemm, whose split-K slabs are per stream, is not called), and every buffer the graph
has baked in belongs to the program or to the object that built it, which outlive the graph."""
import contextlib
import gc
import time

import torch

from . import functional as Fn
from . import hip

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


class StepProgram:
    """One decode step over `rows` rows as zero-argument launches in order (`ops`), with the builders that append to it.  Every buffer
    is allocated while the program is built; finish() closes it."""

    def __init__(self, device, dtype, rows):
        self.device, self.dtype, self.rows = device, dtype, rows
        self.ops = []
        self.weights = []    # (every compute-dtype weight image of the step: held here, so the weight cache cannot drop one mid-call)
        self.shapes = []     # (N, K) of every skinny product, for the shared workspace
        self.stats = self.new(2 * rows, dt=torch.float32)    # LayerNorm's mean | rstd
        self.ws = None

    def new(self, *shape, dt=None):
        return torch.empty(*shape, dtype=dt or self.dtype, device=self.device)

    def add(self, op):
        self.ops.append(op)

    def lin(self, x, weights, biases, out, **epi):
        """out = epilogue(x @ stack(weights)^T + stack(biases)) on the skinny-M kernel; a None among the biases: no bias."""
        w = Fn.fused_weight(list(weights), self.dtype)
        self.weights.append(w)
        biases = list(biases)
        b = None if any(b is None for b in biases) else Fn.fused_bias(biases)
        self.shapes.append(tuple(w.shape))
        fn = Fn.linear_skinny_rows if "step_rows" in epi else Fn.linear_skinny     # (one slot per row: the synthesis stream)
        self.ops.append(lambda: fn(x, w, b, out=out, ws=self.ws, **epi))   # (self.ws: looked up at call time, see finish)
        return out

    def norm(self, ln, x, y):
        self.ops.append(lambda: Fn.layer_norm_into(x, ln.weight, ln.bias, ln.eps, y, self.stats))
        return y

    def finish(self):
        """Behind the last lin: the one skinny-GEMM workspace every product of the step shares."""
        nbytes = max(int(hip.lib().st5_gemm_skinny_ws_bytes(N, K)) for N, K in self.shapes)
        self.ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=self.device)

    def step(self):
        for op in self.ops:
            op()


def append_layers(prog, x, layers, caches, Tmax, counter, self_attn, cross_attn=None, final_norm=None, per_row=False):
    """Appends to `prog` the launches that take x [rows, C] (the newest position of every row) through the decoder `layers` and the
    optional final LayerNorm; returns the buffer that holds the result.  Position = the int32 device scalar `counter`: layer i's K|V go
    to slot `counter` of caches[i] [rows, Tmax, 2C] through the skinny GEMM's device-side output offset.  The attentions are the
    caller's launches, called at step time: self_attn(q, slots, ctx, H, hd) reads positions 0 .. counter of the layer's cache;
    cross_attn(i, q, ctx), when given, is layer i's encoder attention (without it the layers run none: the LM).  Pre- or post-LN per
    layer (normalize_before; a layer without the attribute is pre-LN).  per_row: `counter` is int32 [rows], one position per row (the
    synthesis stream): row b's K|V go to slot counter[b]."""
    lin, norm, new, rows = prog.lin, prog.norm, prog.new, prog.rows
    C = layers[0].self_attn.embed_dim
    for idx, (layer, slots) in enumerate(zip(layers, caches)):
        nb = getattr(layer, "normalize_before", True)
        before = lambda ln, x: norm(ln, x, new(rows, C)) if nb else x      # noqa: E731  (both called inside this iteration only)
        after = lambda ln, x: x if nb else norm(ln, x, new(rows, C))       # noqa: E731
        sa, ca = layer.self_attn, getattr(layer, "encoder_attn", None)
        H, hd = sa.num_heads, sa.head_dim
        # self-attention
        h = before(layer.self_attn_layer_norm, x)
        q = lin(h, [sa.q_proj.weight], [sa.q_proj.bias], new(rows, C))
        lin(h, [sa.k_proj.weight, sa.v_proj.weight], [sa.k_proj.bias, sa.v_proj.bias], slots, step_stride=2 * C, step_cap=Tmax,
            out_ld=Tmax * 2 * C, **({"step_rows": counter} if per_row else {"step": counter}))
        ctx = new(rows, C)
        prog.add(lambda q=q, slots=slots, ctx=ctx, H=H, hd=hd: self_attn(q, slots, ctx, H, hd))
        x = after(layer.self_attn_layer_norm, lin(ctx, [sa.out_proj.weight], [sa.out_proj.bias], new(rows, C), residual=x))
        # cross-attention
        if cross_attn is not None:
            h = before(layer.encoder_attn_layer_norm, x)
            q = lin(h, [ca.q_proj.weight], [ca.q_proj.bias], new(rows, C))
            ctx = new(rows, C)
            prog.add(lambda idx=idx, q=q, ctx=ctx: cross_attn(idx, q, ctx))
            x = after(layer.encoder_attn_layer_norm, lin(ctx, [ca.out_proj.weight], [ca.out_proj.bias], new(rows, C), residual=x))
        # feed-forward
        h = before(layer.final_layer_norm, x)
        f = lin(h, [layer.fc1.weight], [layer.fc1.bias], new(rows, layer.fc1.weight.shape[0]), act=layer.act)
        x = after(layer.final_layer_norm, lin(f, [layer.fc2.weight], [layer.fc2.bias], new(rows, C), residual=x))
    if final_norm is not None:
        x = norm(final_norm, x, new(rows, C))
    return x


def capture(step):
    """`step` captured into a HIP graph on the current stream.  The capture ENQUEUES nothing: the captured step runs for the first time
    at its first replay."""
    torch.cuda.current_stream().synchronize()
    # A graph object freed by the cyclic collector DURING a capture aborts the process.  The collector is switched off for the
    # capture's duration instead of being run in front of it: a full gc.collect() is 26 ... 73 ms per call beside a Base model, the
    # capture itself 1 ... 2 ms (profiles/step_program_timing.txt).
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        graph = torch.cuda.CUDAGraph()
        # capture_begin / capture_end directly: the torch.cuda.graph context would also empty the allocator's cache; the step allocates
        # nothing, so the capture needs no memory pool of its own
        graph.capture_begin(capture_error_mode="thread_local")
        try:
            step()
        except BaseException as first:
            try:                   # the capture is invalid by now and ending it may fail in turn: the step's error is the cause
                graph.capture_end()
            except Exception:
                pass
            raise first
        graph.capture_end()
    finally:
        if gc_was_on:
            gc.enable()
    return graph


def run_steps(step, cap, mode, poll_steps, finished, stats, profile=False):
    """The loop: up to `cap` steps in `mode` ("device": kernel by kernel; "graph": GRAPH_WARMUP_STEPS so, then replays of the captured
    step), grouped by replay_schedule.  Behind a polled group it calls finished() (one host read) and stops when that is true.
    Returns True when a poll ended the loop, False when the schedule ran out (its last group never polls).  `stats` receives polls /
    device_steps / graph_replays (added to what it holds) and, with a capture, capture_s (host clock).  profile: HIP events around
    every group of steps, so that the time of the steps themselves (stats["step_ms"]: device time from the first launch of a group to
    the end of its last kernel, summed over the groups, the capture excluded; stats["steps_timed"]) can be told from the call's set-up
    and capture."""
    graph, spans, at_poll = None, [], False
    try:
        for _first, n_eager, n_replay, poll in replay_schedule(cap, poll_steps, GRAPH_WARMUP_STEPS if mode == "graph" else cap):
            if n_replay and graph is None:
                for _ in range(n_eager):        # (the warm-up steps in front of the capture)
                    step()
                    stats["device_steps"] += 1
                n_eager = 0
                t0 = time.perf_counter()
                graph = capture(step)
                stats["capture_s"] = time.perf_counter() - t0
            if profile:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            for _ in range(n_eager):
                step()
                stats["device_steps"] += 1
            for _ in range(n_replay):
                graph.replay()
                stats["graph_replays"] += 1
            if profile:
                e1.record()
                spans.append((e0, e1, n_eager + n_replay))
            if poll:
                stats["polls"] += 1
                if finished():
                    at_poll = True
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
    return at_poll


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


@contextlib.contextmanager
def on_decode_stream(model, device, mode):
    """Runs the body on the stream of `mode`: decode_stream for "graph" (it never runs on the legacy NULL stream), else the caller's.
    The caller's stream is ordered in front of the body and behind it, so for the caller it behaves like work on its own stream.
    Yields the caller's stream when the body ran on another one -- the tensors it returns then need record_stream(that) -- else None."""
    cur = torch.cuda.current_stream(device)
    side = decode_stream(model, device) if mode == "graph" else cur
    if side != cur:
        side.wait_stream(cur)
    with torch.cuda.stream(side):
        yield cur if side != cur else None
    if side != cur:
        cur.wait_stream(side)
