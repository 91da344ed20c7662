"""One optimizer update as a HIP graph (hipStreamBeginCapture through torch.cuda.CUDAGraph): the step's ~2000 kernel launches
are enqueued once and replayed with a single call, which takes the host (36-48 ms of Python / ctypes enqueue per step, more
than the GPU needs once the kernels are fast) off the critical path and removes the launch gaps between dependent kernels.

What makes a training step replayable:
  * dropout seeds live in device memory (functional.SeedSlots: a `seed` argument with bit 63 set is a pointer, csrc/common.h
    resolve_seed), refilled before every replay with the values the eager path's host counter would have produced;
  * host-produced step inputs (HuBERT span mask and code-book time-mix from the CPU RNGs, target index maps) go through
    functional.stage_host: persistent device buffers + pinned host images, refreshed before every replay in recording order,
    so the numpy / torch CPU random streams advance exactly as in eager mode;
  * data-dependent shapes are replaced by fixed-shape forms while recording (functional.static_shapes(): the NCE head scores
    every frame and passes selection masks; the sample size becomes a device scalar);
  * the optimizer reads the learning rate and step count from device memory (FusedAdam.enable_device_hyper).  Behind the
    finite-gradient guard (FusedAdam(skip_nonfinite=True)) the captured Adam node is st5_adam_step_guard: frozen
    arguments like the others', one guard block for the life of the optimizer; the step count it reads advances by one per replay
    (replay() pushes t + 1, then counts), which the guard block's parity cells rely on.
  * LayerDrop: the per-layer host draws are staged to the device as keep flags and the layer outputs are selected on the
    device (functional.layerdrop_select; modules/encoder.py, modules/decoder.py), so the recipe's --encoder-layerdrop /
    --decoder-layerdrop 0.05 replays (a dropped layer still runs; its output and gradients are discarded).
  * the data: with a BatchFeed the first node of the captured step is st5_batch_load, which copies every tensor leaf of the
    incoming micro-batches into the recorded samples' own tensors (the graph's static inputs); the column of source addresses is
    one more staged input, uploaded with the others (DESIGN.md "Batch feed").
Not supported in a captured step: host reads of device values, collectives.  Several ranks: the captured part is the LOCAL phase of the update (zero_grad, forward / backward of every
micro-batch: ddp.local_phase()), and `after_fn` -- gradient all-reduce + optimizer step -- is enqueued eagerly behind every
replay (a handful of launches)."""
import torch

from . import functional as Fn


# ---------------------------------------------------------------------------------------------------------------------------------
# Batch feed: a new batch for every replayed update
# ---------------------------------------------------------------------------------------------------------------------------------
# Non-tensor values of a sample that only feed logging (or, src_lengths, the feed's own padding mirror) and may therefore differ from
# batch to batch; every other non-tensor value is either equal to the recorded one or the batch is refused (DESIGN.md "Batch feed"
# has the audit: text_pretrain's `ntokens` is the loss divisor, a launch argument of the captured step).
HOST_VALUES_FREE = {
    "speech_pretrain": ("ntokens", "ntokens_list", "nsentences", "src_lengths"),
    "text_pretrain": ("nsentences",),
    # ASR fine-tuning: `ntokens` is free because update.PretrainUpdate only takes an s2t micro-batch under a source when nothing
    # captured reads it -- the criterion divides by B (sentence_avg=True) and logs the pack kernel's count (device_targets=True);
    # DESIGN.md 4m has the audit of every host value of an s2t sample
    "s2t": ("ntokens", "nsentences"),
}
# TTS fine-tuning, in a table of its own: HOST_VALUES_FREE keeps the entries it had (tests/test_ctc_pack_cpu.py pins that it does not
# name t2s).  `ntokens` only feeds the log; with the criterion's device_ntokens=True the log takes src_lengths.sum() off the device
# instead (update.check_t2s_source).  `nsentences` is B, a function of the signature.  DESIGN.md 4p has the audit
HOST_VALUES_FREE_T2S = {
    "t2s": ("ntokens",),
}


def host_values_free():
    """{task name: host values of a sample that may differ from batch to batch}: both tables, what BatchFeed.check and the statistics
    audit (train_stats.check_feed_host_values) go by."""
    return {**HOST_VALUES_FREE, **HOST_VALUES_FREE_T2S}
# keys a criterion writes into the sample it is given (criterions.py: dec_weight == 0, ce_weight == 0): not part of a batch
CRITERION_WRITTEN = ("net_input.only_hubert", "only_ctc")


def _path(i, keys):
    return f"micro_batches[{i}]" + "".join(f"[{k}]" if isinstance(k, int) else f".{k}" for k in keys)


def flatten_sample(sample):
    """{key path (tuple): leaf} of a nested sample: dicts by key, lists / tuples that hold a tensor or a container by index; any other
    value (a number, a string, a list of numbers, None) is a leaf."""
    out = {}

    def walk(x, keys):
        if isinstance(x, dict):
            for k, v in x.items():
                walk(v, keys + (k,))
        elif isinstance(x, (list, tuple)) and any(torch.is_tensor(v) or isinstance(v, (dict, list, tuple)) for v in x):
            for k, v in enumerate(x):
                walk(v, keys + (k,))
        else:
            out[keys] = x
    walk(sample, ())
    return out


def batch_signature(micro_batches):
    """What a replayed update fixes about its data: per micro-batch the task name and, per tensor leaf, key path, shape and dtype."""
    sig = []
    for s in micro_batches:
        flat = flatten_sample(s)
        sig.append((s.get("task_name"), tuple(sorted((".".join(map(str, k)), tuple(v.shape), str(v.dtype)) for k, v in flat.items() if torch.is_tensor(v)))))
    return tuple(sig)


def _same_host_value(a, b):
    if type(a) is not type(b) and not (isinstance(a, (int, float)) and isinstance(b, (int, float))):
        return False
    try:
        return bool(a == b)
    except Exception:
        return False


def padding_mirror(sample, i=0):
    """The speech padding mask of a sample on the host without reading the device: the `_st5_host` the batch carries on the mask
    (collate.SpeechPretrainCollater attaches it), else built from the sample's host `src_lengths` list (row b is padded from
    src_lengths[b] on).  None for a sample without a padding mask."""
    pm = sample.get("net_input", {}).get("padding_mask") if isinstance(sample.get("net_input"), dict) else None
    if pm is None:
        return None
    host = getattr(pm, "_st5_host", None)
    if host is not None:
        if not (torch.is_tensor(host) and host.device.type == "cpu" and host.dtype == torch.bool and tuple(host.shape) == tuple(pm.shape)):
            raise ValueError(f"{_path(i, ('net_input', 'padding_mask'))}: its host copy (_st5_host) is not a CPU bool tensor of shape {tuple(pm.shape)}")
        return host
    n = sample.get("src_lengths")
    if torch.is_tensor(n) and n.device.type == "cpu":
        n = n.tolist()
    if not isinstance(n, (list, tuple)) or len(n) != pm.shape[0] or not all(isinstance(v, int) and 0 <= v <= pm.shape[1] for v in n):
        raise ValueError(f"{_path(i, ('src_lengths',))}: the padding mask's host copy is built from a host list of {pm.shape[0]} lengths in "
                         f"[0, {pm.shape[1]}] (or carried by the mask as _st5_host, as the collater does); got {n!r}")
    return torch.arange(pm.shape[1])[None, :] >= torch.tensor(list(n), dtype=torch.long)[:, None]


class _Pulled:
    __slots__ = ("batch", "leaves", "ptrs", "ready", "host", "mirrors")


class BatchFeed:
    """Connects a source of batches to a recorded step.  `static` -- the micro-batches the step is recorded on -- fixes the batch
    signature; their tensors are the graph's static inputs and are OVERWRITTEN by every load.  pull() takes the next element of the
    source on the calling thread, checks it against the signature (ValueError naming the path: other keys, shape, dtype, task_name, a
    leaf on another device, a host value the captured step has baked in), makes a contiguous copy where needed, records an event
    behind the batch's producer and re-points the host side of the static samples (logging values, the padding mask's mirror) at it.
    load() is what the step calls first: one st5_batch_load from the pulled batch's leaves into the static tensors, the source
    addresses a staged input.  No method reads device memory."""

    def __init__(self, static, device=None):
        self.static = list(static)
        self.signature = batch_signature(self.static)
        self.paths, self.dst, self.host_paths = [], [], []
        self._flat = []            # per micro-batch {key path: leaf} as RECORDED (pull() re-points the samples, not this)
        for s in self.static:
            self._flat.append({k: v for k, v in flatten_sample(s).items() if ".".join(map(str, k)) not in CRITERION_WRITTEN})
        if device is None:         # where the step runs: the first tensor off the host decides (all on the host: tests)
            off = [v.device for flat in self._flat for v in flat.values() if torch.is_tensor(v) and v.device.type != "cpu"]
            device = off[0] if off else torch.device("cpu")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        for i, flat in enumerate(self._flat):
            for k, v in flat.items():
                if torch.is_tensor(v) and v.device == self.device:      # a leaf the load copies
                    if not v.is_contiguous():
                        raise ValueError(f"{_path(i, k)}: a static input of the recorded step must be contiguous")
                    self.paths.append((i, k))
                    self.dst.append(v)
                elif torch.is_tensor(v) and v.device.type != "cpu":
                    raise ValueError(f"{_path(i, k)}: on {v.device}, the update runs on {self.device}")
                else:                                                   # a host value or a CPU tensor (id, sort_order)
                    self.host_paths.append((i, k))
        self.nbytes = [v.numel() * v.element_size() for v in self.dst]
        self.prefix = Fn.batch_load_plan(self.nbytes)
        self.n_leaves, self.total_chunks = len(self.dst), self.prefix[-1]
        self._table = None         # device int64 [3 n + 1]: destinations, byte counts, chunk prefix -- written once (load())
        self.source = None
        self.caller_stream = None  # the stream pull() runs the source on (update.PretrainUpdate.update sets it); None: the current one
        self.pulled = None         # the batch the next produced step trains on
        self.in_slot = [None, None]   # the batch whose addresses were produced into each pinned slot
        self.held = []             # [(batch record, event behind the work that read it)]
        self.pulls = 0

    # -- source ---------------------------------------------------------------------------------------------------------------
    def set_source(self, iterable):
        self.source = iter(iterable)

    def check(self, batch):
        """The incoming batch against the recorded signature -> ([leaf tensors in table order], {host path: value}, [mirror per
        micro-batch]); raises ValueError, and changes nothing, for a batch the captured step cannot take."""
        if not isinstance(batch, (list, tuple)) or len(batch) != len(self.static):
            raise ValueError(f"a batch is a list of {len(self.static)} micro-batches, got {type(batch).__name__}"
                             + (f" of {len(batch)}" if isinstance(batch, (list, tuple)) else ""))
        flats = []
        for i, (s, ref) in enumerate(zip(batch, self._flat)):
            if not isinstance(s, dict):
                raise ValueError(f"micro_batches[{i}]: not a sample dictionary")
            name, want = s.get("task_name"), self.static[i].get("task_name")
            if name != want:
                raise ValueError(f"{_path(i, ('task_name',))}: {name!r}, the step was recorded on {want!r}")
            flat = {k: v for k, v in flatten_sample(s).items() if ".".join(map(str, k)) not in CRITERION_WRITTEN}
            for k in ref:
                if k not in flat:
                    raise ValueError(f"{_path(i, k)}: missing from the batch (the recorded signature has it)")
            for k in flat:
                if k not in ref:
                    raise ValueError(f"{_path(i, k)}: not in the recorded signature")
            flats.append(flat)
        leaves = []
        for (i, k), d in zip(self.paths, self.dst):
            v = flats[i][k]
            if not torch.is_tensor(v):
                raise ValueError(f"{_path(i, k)}: a {type(v).__name__}, the recorded signature has a tensor")
            if v.device != d.device:
                raise ValueError(f"{_path(i, k)}: on {v.device}, the recorded step reads {d.device}")
            if v.dtype != d.dtype or tuple(v.shape) != tuple(d.shape):
                raise ValueError(f"{_path(i, k)}: {tuple(v.shape)} {v.dtype}, the recorded signature has {tuple(d.shape)} {d.dtype} "
                                 "(nothing is padded or cropped)")
            leaves.append(v)
        host = {}
        for i, k in self.host_paths:
            v, ref = flats[i][k], self._flat[i][k]
            if torch.is_tensor(ref):      # a CPU tensor of the sample (id, sort_order): read for its shape and by logging only
                if not (torch.is_tensor(v) and v.device == ref.device and v.dtype == ref.dtype and tuple(v.shape) == tuple(ref.shape)):
                    what = f"{tuple(v.shape)} {v.dtype} on {v.device}" if torch.is_tensor(v) else type(v).__name__
                    raise ValueError(f"{_path(i, k)}: {what}, the recorded signature has {tuple(ref.shape)} {ref.dtype} on {ref.device}")
            elif torch.is_tensor(v):
                raise ValueError(f"{_path(i, k)}: a tensor, the recorded signature has a {type(ref).__name__}")
            elif k != ("task_name",) and not (len(k) == 1 and k[0] in host_values_free().get(self.static[i].get("task_name"), ())) \
                    and not _same_host_value(v, ref):
                raise ValueError(f"{_path(i, k)}: {v!r}, the step was recorded with {ref!r} -- a host value that reaches "
                                 "a captured launch (for text_pretrain's ntokens: the loss divisor) cannot change between replays")
            host[(i, k)] = v
        mirrors = [padding_mirror(s, i) for i, s in enumerate(batch)]
        return leaves, host, mirrors

    def _overlaps(self, leaves):
        spans = [(d.data_ptr(), d.data_ptr() + n) for d, n in zip(self.dst, self.nbytes) if n]
        for (i, k), v, d, n in zip(self.paths, leaves, self.dst, self.nbytes):
            a = v.data_ptr()
            if n == 0 or a == d.data_ptr():      # (the static tensor itself: every byte is rewritten with its own value)
                continue
            if any(a < hi and lo < a + n for lo, hi in spans):
                raise ValueError(f"{_path(i, k)}: shares memory with a static input of the recorded step")

    def pull(self, for_eager=False):
        """The next batch of the source, checked; StopIteration when the source has ended (nothing is changed then)."""
        if self.source is None:
            raise RuntimeError("BatchFeed.pull() without a source")
        on = self.caller_stream if (self.caller_stream is not None and self.device.type == "cuda") else None
        ctx = torch.cuda.stream(on) if on is not None else _Null()
        with ctx:
            batch = next(self.source)
            self.pulls += 1
            if for_eager:      # (run as it is, on its own tensors: no captured step fixes anything about it)
                if not isinstance(batch, (list, tuple)) or not all(isinstance(b, dict) for b in batch):
                    raise ValueError("a batch is a list of micro-batches (sample dictionaries)")
                leaves, host, mirrors = [], {}, []
            else:
                leaves, host, mirrors = self.check(batch)
                leaves = [v if v.is_contiguous() else v.contiguous() for v in leaves]     # (a copy on the caller's thread and stream)
                self._overlaps(leaves)
            rec = _Pulled()
            rec.batch, rec.leaves, rec.host, rec.mirrors = batch, leaves, host, mirrors
            rec.ptrs = torch.tensor([v.data_ptr() for v in leaves], dtype=torch.int64)
            rec.ready = None
            if self.device.type == "cuda":
                rec.ready = torch.cuda.Event()
                rec.ready.record()          # behind the batch's producer (the collater's launches on this stream)
        if for_eager:     # (the pre-net takes the mirror the batch carries, else reads the mask once: always the batch's own)
            return rec
        # the host side of the static samples now describes this batch: logging values, CPU tensors, the padding mask's mirror
        for (i, k), v in host.items():
            node = self.static[i]
            for key in k[:-1]:
                node = node[key]
            node[k[-1]] = v
        for s, m in zip(self.static, mirrors):
            if m is not None:
                s["net_input"]["padding_mask"]._st5_host = m
        self.pulled = rec
        return rec

    # -- the step's side --------------------------------------------------------------------------------------------------------
    def _addresses(self):
        return self.pulled.ptrs

    def mark(self, slot):
        """(host only) the step just produced into pinned slot `slot` trains on the pulled batch."""
        self.in_slot[slot] = self.pulled

    def table(self):
        if self._table is None:
            n = self.n_leaves
            t = torch.tensor([d.data_ptr() for d in self.dst] + self.nbytes + self.prefix, dtype=torch.int64).to(self.device)
            self._table = (t, t[:n], t[n:2 * n], t[2 * n:])
        return self._table

    def load(self):
        """First launch of the recorded / captured step: the pulled batch into the static tensors.  Recording: enqueued now, behind
        the batch's producer.  Capturing: the node only; its source addresses arrive with the staged block before every replay."""
        if self.total_chunks == 0:
            return
        mode = Fn.staging.mode
        if mode != "capture" and self.pulled.ready is not None:
            torch.cuda.current_stream(self.device).wait_event(self.pulled.ready)
        col = Fn.stage_host(self._addresses, self.device)
        _, dst, nbytes, prefix = self.table()
        Fn.batch_load(col, dst, nbytes, prefix, self.n_leaves, self.total_chunks)

    def before_launch(self, slot):
        """The replay that reads pinned slot `slot`'s addresses waits for that batch's producer."""
        rec = self.in_slot[slot]
        if rec is not None and rec.ready is not None:
            torch.cuda.current_stream(self.device).wait_event(rec.ready)
        return rec

    def retire(self, rec):
        """`rec` has been read by work enqueued on the current stream: its tensors stay referenced until that work has completed."""
        if rec is None or self.device.type != "cuda":
            return
        ev = torch.cuda.Event()
        ev.record()
        self.held = [(r, e) for r, e in self.held if not e.query()]
        self.held.append((rec, ev))


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class ReplaySchedule:
    """The host-side order of a replay loop, apart from anything that touches the device: when the source is pulled, when a step's
    host inputs are produced (its random draws), when they are uploaded -- with and without the helper thread.  Callables:
    produce(slot) (host only; runs on the helper thread under prefetch), upload(slot), slot_free(slot) (returns once the previous
    upload from that pinned slot has executed), pull() or None (the batch feed: raises StopIteration when the source has ended).

    Order: pull k, produce k, pull k + 1, produce k + 1 ...: a pull happens on the calling thread, after the previous helper thread
    is joined and before the next one starts, so the host random streams (the collater's crop starts and the BART noise are drawn
    inside the pull) advance as in an eager loop.  Under prefetch batch k + 1 is pulled during begin() k.  When that pull ends the
    source (or refuses the batch), step k -- already prepared -- still runs, no helper is started (no unused step's draws are
    consumed) and the NEXT begin() raises what the pull raised."""

    def __init__(self, produce, upload, pull=None, prefetch=False, slot_free=None):
        self.produce, self.upload, self.pull, self.prefetch = produce, upload, pull, prefetch
        self.slot_free = slot_free if slot_free is not None else (lambda slot: None)
        self._pending = False
        self._ahead = None      # (thread, slot) preparing the next step
        self._ahead_error = None
        self._pull_error = None
        self._slot = 0

    def _prepare_here(self):
        self.slot_free(0)
        self.produce(0)
        self.upload(0)

    def prime(self):
        """(capture) the first replay's batch and host inputs, staged now."""
        if self.pull is not None:
            self.pull()
        self._prepare_here()
        self._pending = True

    def new_source(self):
        self._pull_error = None

    def begin(self):
        """Everything in front of a replay's launch; returns the pinned slot this step's inputs came from."""
        if self._pull_error is not None:
            raise self._pull_error
        used = 0
        if self._pending:
            self._pending = False
        elif self._ahead is not None:
            th, used = self._ahead
            th.join()
            self._ahead = None
            if self._ahead_error is not None:
                raise self._ahead_error
            self.upload(used)
        else:
            if self.pull is not None:
                self.pull()
            self._prepare_here()
        if self.prefetch:
            import threading
            self._slot = used ^ 1      # (the other pinned image: never the one this step's upload reads)
            self._ahead_error = None
            self.slot_free(self._slot)
            if self.pull is not None:
                try:
                    self.pull()
                except BaseException as e:     # (StopIteration: the source has ended) surfaced by the next begin()
                    self._pull_error = e
                    return used

            def work(slot=self._slot):
                try:
                    self.produce(slot)
                except BaseException as e:   # surfaced by the next begin()
                    self._ahead_error = e
            th = threading.Thread(target=work, daemon=True)
            th.start()
            self._ahead = (th, self._slot)
        return used

    def drain(self):
        if self._ahead is not None:
            self._ahead[0].join()


class StepGraph:
    def __init__(self, step_fn, opt=None, model=None, device=None, seed_slots=1024, on_step=None, prefetch_host=False, after_fn=None,
                 stream=None, phases=None, between=None, feed=None):
        """step_fn(): one full update on the current stream -- zero_grad, forward/backward of every micro-batch, finish,
        optimizer step -- without host synchronisation.  `opt`: the FusedAdam whose (lr, step) must follow the host.
        after_fn(): optional eager tail of the update, NOT captured (then step_fn must not contain the optimizer step: after_fn
        does, after the collectives).  feed: a BatchFeed with a source -- every recorded step and every replay then trains on the next
        batch of the source; its load is the first launch of the step (of the first phase)."""
        # phases / between (several ranks, overlapped exchange): the update's local part as a LIST of callables, each captured
        # into its own graph (one memory pool, replayed in order), and after each of them an eagerly enqueued callable -- the
        # asynchronous all-reduce of the bucket range that phase completed -- so the collective runs on the process group's
        # stream while the next phase's graph executes.  step_fn is then None.
        self.phases = list(phases) if phases is not None else None
        self.between = list(between) if between is not None else None
        assert self.phases is None or (step_fn is None and len(self.phases) == len(self.between))
        self.graphs = None
        self.step_fn = step_fn
        self.after_fn = after_fn
        self.on_step = on_step   # host-side bookkeeping a replay skips (e.g. model.set_num_updates(n)): called before every step
        self.opt = opt
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.graph = None
        self._assumes_zeroed = False
        # prefetch_host: hipGraphLaunch keeps the calling thread until the previous launch of the same graph has drained (measured:
        # graph.replay() returns after 40-60 ms), so the host part of the NEXT step's preparation (on_step, seed values, the CPU
        # producers of the staged inputs: ~1.2 ms) would sit between two replays with the GPU idle.  With prefetch_host it runs on
        # a helper thread while the launch call blocks (the call releases the GIL), into the second pinned image of every staged
        # buffer; replay() then only enqueues the uploads.  The CPU random streams are drawn in the same order, one step EARLIER
        # than without (after the last replay one prepared, unused step has advanced them).
        self.prefetch_host = prefetch_host
        self.feed = feed
        # who pulls, produces and uploads when (ReplaySchedule): host-only logic, tests/test_batch_feed_cpu.py drives it with stubs
        self.sched = ReplaySchedule(self._produce, self._upload, pull=feed.pull if feed is not None else None, prefetch=prefetch_host,
                                    slot_free=self._slot_free)
        self._lr = [None, None]  # the learning rate on_step() left behind, per pinned slot (read on the thread that ran on_step)
        self.trace = None        # tests: a list -> one record per replay of what was uploaded (digests of the pinned images)
        self._uploaded = [None, None]   # event after the last upload from each pinned slot (the slot may be rewritten only after it)
        self.slots = Fn.SeedSlots(seed_slots, self.device)
        self.staging = Fn.HostStaging()   # per graph: two graphs (two tests, two shapes) never share a staging sequence
        self.stream = stream if stream is not None else torch.cuda.Stream(device=self.device)   # (never the NULL stream)
        if opt is not None and opt.hyper_dev is None:
            opt.enable_device_hyper()

    # -- one step in a given staging mode ------------------------------------------------------------------------------
    def _enter(self, mode):
        Fn._S.slots = self.slots
        self._prev_staging, Fn.staging = Fn.staging, self.staging     # this graph's own sequence of staged inputs / host draws
        self.staging.begin_step(mode)

    def _exit(self):
        Fn._S.slots = None
        self.staging.mode = None
        Fn.staging = self._prev_staging

    def _run(self, mode):
        self._enter(mode)
        try:
            if self.feed is not None:
                self.feed.load()         # (the first launch of the step / of the first phase)
            if self.phases is None:
                self.step_fn()
            else:
                for fn, bt in zip(self.phases, self.between):
                    fn()
                    if mode == "record":
                        bt()
        finally:
            self._exit()

    def record(self):
        """Eager step that allocates the static buffers and counts the seed slots (also the last warm-up step)."""
        # on the capture stream: per-stream state of the library (split-K slab workspaces) and of the allocator is created
        # here, eagerly -- nothing may allocate device memory once capture has begun
        cur = torch.cuda.current_stream(self.device)
        rec = self.feed.pull() if self.feed is not None else None      # (before the step's host draws, as in every later step)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            if self.on_step is not None:
                self.on_step()
            if self.opt is not None:
                self.opt.push_hyper()
            self.slots.begin_step()
            self._run("record")
            if self.after_fn is not None:
                self.after_fn()
            if self.feed is not None:
                self.feed.retire(rec)
        cur.wait_stream(self.stream)
        if not self.slots.used:
            self.slots.used = self.slots.k
            Fn._S.counter -= self.slots.n - self.slots.used   # begin_step() reserved all slots: give the unused ones back
        else:
            assert self.slots.k == self.slots.used, "the step's dropout call sequence changed"

    def capture(self):
        torch.cuda.synchronize(self.device)
        self.staging.pack()      # (all staged inputs in one block: one upload per replay instead of one per tensor)
        with torch.cuda.stream(self.stream):
            self.sched.prime()       # (pulls the first replay's batch, produces and uploads its host inputs)
        torch.cuda.synchronize(self.device)
        import gc
        gc.collect()    # (a graph object freed by the cyclic collector DURING a capture aborts the process)
        self.graph = torch.cuda.CUDAGraph()
        t0 = self.opt.t if self.opt is not None else 0
        # does the captured zero_grad() contain the fills, or does it rely on the previous optimizer step having left the
        # gradient buffers zeroed (ddp._grads_zeroed at this moment)?  replay() re-establishes that precondition when the host
        # flag says the buffers were written in between (an eager backward without a step, a failed step ...)
        ddp = getattr(self.opt, "ddp", None)
        self._assumes_zeroed = bool(ddp is not None and ddp._grads_zeroed)
        try:
            if self.phases is None:
                with torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
                    self._run("capture")
            else:
                pool = torch.cuda.graph_pool_handle()
                self.graphs = []
                self._enter("capture")
                try:
                    for k, fn in enumerate(self.phases):
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g, pool=pool, stream=self.stream, capture_error_mode="thread_local"):
                            if k == 0 and self.feed is not None:
                                self.feed.load()
                            fn()
                        self.graphs.append(g)
                finally:
                    self._exit()
        except BaseException:
            # a failed capture usually ends the process in the graph's destructor ("operation not permitted when stream is
            # capturing") before Python prints the cause: show it here, while the graph object is still referenced
            import sys
            import traceback
            traceback.print_exc()
            sys.stderr.flush()
            raise
        # the capture pass itself executed nothing: the host-side step counter it advanced is rolled back
        if self.opt is not None and self.after_fn is None:
            self.opt.t = t0
        assert self.slots.k == self.slots.used, "the captured step used a different number of dropout seeds than the recorded one"
        if self.prefetch_host:
            # every pinned image the helper thread will write exists before it first runs: the helper never allocates pinned
            # memory (hipHostMalloc from a second host thread beside a graph launch) and never touches the HIP runtime at all
            self.slots.ensure_second_image()
            self.staging.ensure_second_images()
            if self.opt is not None:
                self.opt.ensure_second_hyper_image()

    def _produce(self, slot):
        """Host half of the preparation of one step (no device work)."""
        if self.on_step is not None:
            self.on_step()
        if self.opt is not None:
            self._lr[slot] = float(self.opt.lr)   # (snapshot on the producing thread: the upload never reads a half-advanced schedule)
        if self.feed is not None:
            self.feed.mark(slot)    # (host only: which batch's addresses this slot's image holds)
        self.slots.produce(slot)
        self.staging.produce(slot)

    def _upload(self, slot):
        self.slots.upload(slot)
        self.staging.upload(slot)
        if self.opt is not None:
            self.opt.push_hyper(slot, lr=self._lr[slot])
        if self.trace is not None:
            self.trace.append({"slot": slot, "seeds": self.slots.digest(slot), "staged": self.staging.digests(slot),
                               "lr": self._lr[slot], "t": (self.opt.t + 1) if self.opt is not None else None})
        # the uploads are asynchronous reads of pinned host images: remember when this slot's have executed (a host that runs
        # ahead of the GPU -- small steps -- must not rewrite the images before that)
        ev = torch.cuda.Event()
        ev.record()
        self._uploaded[slot] = ev

    def _slot_free(self, slot):
        if self._uploaded[slot] is not None:
            self._uploaded[slot].synchronize()

    def _pre_replay(self):
        self._slot_free(0)
        self._produce(0)
        self._upload(0)

    def replay(self):
        """One replayed update.  It is ALWAYS enqueued on this graph's own stream (uploads of the staged inputs, the graph
        launch, the eager tail), whatever stream the caller is on -- in particular never on the legacy NULL stream, which this
        runtime does not keep in issue order when more than one host thread is alive beside it; the
        caller's stream is ordered before and behind the replay, so for the caller it behaves like work on its own stream."""
        cur = torch.cuda.current_stream(self.device)
        if cur == self.stream:
            return self._replay()
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            self._replay()
        cur.wait_stream(self.stream)

    def _replay(self):
        used = self.sched.begin()     # the pinned slot this step's inputs came from (ReplaySchedule has the order of events)
        step_lr = self._lr[used]
        rec = self.feed.before_launch(used) if self.feed is not None else None
        ddp = getattr(self.opt, "ddp", None)
        if self._assumes_zeroed and ddp is not None and not ddp._grads_zeroed:
            ddp.flat.zero_()
            if ddp.flat2 is not None:
                ddp.flat2.zero_()
            ddp._pair_pending = False
        if self.graphs is not None:
            for g, bt in zip(self.graphs, self.between):
                g.replay()
                bt()
        else:
            self.graph.replay()
        if self.after_fn is not None:
            # the eager tail's optimizer step passes lr BY VALUE; by now the helper thread may have advanced the schedule to the
            # next step (on_step runs one step early there): the tail reads this step's snapshot
            if self.opt is not None:
                self.opt.lr_step = step_lr
            try:
                self.after_fn()          # (its optimizer step advances opt.t itself)
            finally:
                if self.opt is not None:
                    self.opt.lr_step = None
        elif self.opt is not None:
            self.opt.t += 1
            if ddp is not None:
                ddp._grads_zeroed = True     # the replayed Adam kernel left both buffers zeroed
        if self.feed is not None:
            self.feed.retire(rec)            # (the batch stays referenced until an event behind this replay has completed)

    def drain(self):
        """Wait for the helper thread that prepares the next step (prefetch_host): after the last replay it has drawn one unused
        step's worth of host random numbers; whoever re-seeds the CPU generators afterwards must not race with it."""
        self.sched.drain()

    def __call__(self):
        if self.graph is None:
            self.record()
            self.record()   # second recording step: confirms that the slot / staging sequence repeats
            self.capture()
        self.replay()
