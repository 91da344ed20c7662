"""Training statistics from the replayed update (update.PretrainUpdate(stats=True)).

The trainer the reference runs under reads every entry of the criterion's logging output with `.item()` after every update and hands
the list to `reduce_metrics`.  A replayed update has no such Python: the logged scalars are device tensors inside the captured graph's
private pool.  StatsRecorder is their way out without a host synchronisation:

  * at the first update it fixes the CELL LAYOUT: per micro-batch every entry of the aggregated logging output that is a one-element
    device tensor (key path kept, e.g. `micro[0].speech_pretrain.loss_m_0`), plus `opt.gnorm_sq` when the update clips -- and, for
    an update behind the finite-gradient guard (PretrainUpdate(nonfinite="skip")), `opt.gnorm_sq` in any case and
    `opt.skipped`, the flag cell of the optimizer's guard block: one more descriptor of the same launch;
  * every update ends with ONE st5_stats_record launch (csrc/train_stats.hip) that copies the scalars, widened to 8-byte cells, into
    row `counter % rows` of a device ring behind the stamp `counter` -- eagerly enqueued, recorded or as the last node of the captured
    graph, always the same kernel on the same ring;
  * every rows // 2 updates the calling thread enqueues one asynchronous copy of the whole ring into one of two alternating pinned
    images, with an event behind it (HarvestSchedule: host-only, tests/test_train_stats_cpu.py drives it with stubs);
  * harvest() turns the rows of every image whose event has completed into the dictionaries `train_step(sync=True)` returns.

Entries of the log that are host numbers are kept as host values: those of the step that was enqueued, and for a replay those of the
captured pass (functions of the batch signature, or values the batch feed refuses to let differ: DESIGN.md 4k has the audit)."""
import math

import torch

from . import functional as Fn

# type codes of csrc/train_stats_index.h (TS_F32 ...)
TYPE_CODES = {torch.float32: 0, torch.float64: 1, torch.bfloat16: 2, torch.float16: 3, torch.int64: 4, torch.int32: 5, torch.uint8: 6,
              torch.bool: 6}
MAX_CELLS = 1024      # TS_MAX_CELLS

# Logged entries that are a SAMPLE's host value, per task name: {logging key: key of the sample}.  Every other host-valued entry of the
# criteria in criterions.py is a function of the batch signature (a tensor's shape) or a constant.  Under a batch feed a
# replay reports the captured pass's host values, so a sample value logged here must be one graph.BatchFeed refuses to let differ.
LOGGED_SAMPLE_VALUES = {
    "speech_pretrain": {},
    "text_pretrain": {"ntokens": "ntokens", "sample_size": "ntokens"},
    "t2s": {"ntokens": "ntokens"},
    "s2s": {"ntokens": "ntokens"},
    "s2t": {"ntokens": "ntokens", "sample_size": "ntokens"},
    "s2c": {"ntokens": "ntokens", "sample_size": "ntokens"},
}


# Entries of LOGGED_SAMPLE_VALUES that a criterion OPTION takes off the host: {task name: {logging key: how}}.  The s2t criterion
# with device_targets=True logs the pack kernel's label count as `ntokens` (a device cell), and with sentence_avg=True its
# `sample_size` is B, a function of the batch signature.  The t2s criterion with device_ntokens=True logs src_lengths.sum(), a device
# scalar.  check_feed_host_values skips exactly the keys its caller names.
DEVICE_LOGGED_OPTIONS = {
    "s2t": {"ntokens": "device_targets=True", "sample_size": "sentence_avg=True"},
    "t2s": {"ntokens": "device_ntokens=True"},
}


def device_logged(task_name, criterion):
    """The logging keys of LOGGED_SAMPLE_VALUES[task_name] that `criterion` (a SpeechT5Criterion, or the task's own criterion) does
    not take from the sample's host value, as check_feed_host_values' `device_logged` entry for that task."""
    if task_name == "t2s":
        c = getattr(criterion, "speech_criterion", criterion)
        return ("ntokens",) if getattr(c, "device_ntokens", False) else ()
    if task_name != "s2t":
        return ()
    c = getattr(criterion, "text_criterion", criterion)
    keys = []
    if getattr(c, "device_targets", False):
        keys.append("ntokens")
    if getattr(c, "sentence_avg", False):
        keys.append("sample_size")
    return tuple(keys)


def check_feed_host_values(task_names, free, device_logged=None):
    """Refuse, by name, a criterion whose log carries a sample's host value that the feed lets vary per batch (`free`:
    graph.HOST_VALUES_FREE): a replay would report the captured pass's value for every batch.  device_logged: {task name: logging
    keys the criterion at hand does NOT take from the host} (DEVICE_LOGGED_OPTIONS names the options; device_logged() reads them off
    a criterion) -- those keys are not checked; a key outside DEVICE_LOGGED_OPTIONS is refused."""
    device_logged = device_logged or {}
    for name, keys in device_logged.items():
        for key in keys:
            if key not in DEVICE_LOGGED_OPTIONS.get(name, {}):
                raise ValueError(f"stats: no option of the {name} criterion is known to keep `{key}` off the host "
                                 "(train_stats.DEVICE_LOGGED_OPTIONS)")
    for i, name in enumerate(task_names):
        if name not in LOGGED_SAMPLE_VALUES:
            raise ValueError(f"stats: micro_batches[{i}].task_name {name!r}: no audit of this criterion's host-valued logging entries "
                             "(train_stats.LOGGED_SAMPLE_VALUES); it cannot be replayed under a source with stats=True")
        for key, src in LOGGED_SAMPLE_VALUES[name].items():
            if key in device_logged.get(name, ()):
                continue
            if src in free.get(name, ()):
                raise ValueError(f"stats: the {name} criterion logs `{key}` from the sample's host value `{src}`, which the batch feed lets "
                                 "differ from batch to batch; a replayed update cannot report it")


def cell_path(i, keys):
    return f"micro[{i}]." + ".".join(map(str, keys))


class HarvestSchedule:
    """When the ring is copied to the host, into which image, and which rows a completed image contributes -- nothing here touches the
    device.  Callables: copy(image) -> token (enqueues the copy of the whole ring into pinned image 0 / 1 and an event behind it),
    done(token) -> bool (no wait), wait(token), read(image, row) -> (stamp, payload) (the payload detached from the image).

    updated() is called once per update, after its record launch was enqueued (ordinals 1, 2, ...).  Every rows // 2 updates it copies
    into the image the previous copy did not use; an image still waiting to be harvested is harvested first (and only then waited
    for: the host would have to be a whole ring ahead of the device).  A copy made after update k holds updates k - rows + 1 .. k, so
    with a copy every rows // 2 updates each row is copied at least once before it is overwritten.  harvest() takes completed images
    in copy order and checks every row's stamp (the update counter the kernel wrote, ordinal - 1) against the ordinal it delivers."""

    def __init__(self, rows, copy, done, wait, read):
        if not (isinstance(rows, int) and rows >= 2):
            raise ValueError(f"stats_rows = {rows!r}: the ring has at least 2 rows")
        self.rows, self.every = rows, rows // 2
        self.copy, self.done, self.wait, self.read = copy, done, wait, read
        self.enqueued = 0       # updates whose record launch has been enqueued
        self.copied = 0         # the newest update an enqueued copy holds
        self.delivered = 0      # the newest update taken out of an image
        self.pending = []       # [(image, token, newest update in it)] in copy order
        self.image = 0          # the image the next copy goes to
        self.ready = []         # [(ordinal, payload)] taken, not yet handed out

    def updated(self):
        self.enqueued += 1
        if self.enqueued % self.every == 0:
            self._copy()

    def _copy(self):
        while any(img == self.image for img, _, _ in self.pending):
            self._take(wait=True)
        self.pending.append((self.image, self.copy(self.image), self.enqueued))
        self.copied = self.enqueued
        self.image ^= 1

    def _take(self, wait):
        img, token, upto = self.pending[0]
        if wait:
            self.wait(token)
        elif not self.done(token):
            return False
        if upto - self.delivered > self.rows:
            raise RuntimeError(f"stats ring: updates {self.delivered + 1} to {upto - self.rows} were overwritten before a copy held them")
        for k in range(self.delivered + 1, upto + 1):
            stamp, payload = self.read(img, (k - 1) % self.rows)
            if stamp != k - 1:
                raise RuntimeError(f"stats ring: row {(k - 1) % self.rows} holds the stamp {stamp}, update {k} expects {k - 1}")
            self.ready.append((k, payload))
        self.delivered = max(self.delivered, upto)
        self.pending.pop(0)
        return True

    def harvest(self):
        """[(ordinal, payload)] of every completed image, in update order; never waits."""
        while self.pending and self._take(wait=False):
            pass
        out, self.ready = self.ready, []
        return out

    def drain(self):
        """One more copy when updates were enqueued behind the last one, then every image waited for: the next harvest() has all."""
        if self.enqueued > self.copied:
            self._copy()
        while self.pending:
            self._take(wait=True)


class StatsRecorder:
    def __init__(self, device, rows=64, clip_norm=0.0, grad_scale=1.0, guard=False):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.clip_norm, self.grad_scale = float(clip_norm), float(grad_scale)
        self.guard = bool(guard)    # the optimizer steps behind st5_adam_step_guard: its flag cell is logged as `skipped`
        self.sched = HarvestSchedule(rows, self._copy_ring, lambda ev: ev.query(), lambda ev: ev.synchronize(), self._read_row)
        self.rows = rows
        self.layout = None          # [(micro-batch, key path, "cell" | "host", dtype | None)] in the order of the logging output
        self.cell_types = []        # dtype per cell, in cell order
        self.paths = []             # key path string per cell
        self.n_cells = 0
        self.gnorm_cell = self.skipped_cell = None
        self.ring = self.counter = self.images = self.addr_dev = self.types_dev = None
        self._addr_host = None      # two pinned images of the address column for eagerly enqueued steps
        self._addr_event = [None, None]
        self._addr_slot = 0
        self._graph_addr = None     # pinned: the capture-time addresses (constant over replays: the graph's pool)
        self._graph_hosts = None
        self._dev_is_graph = False  # the device column holds the capture-time addresses
        self._held = None           # logged tensors of the captured pass, until the capture has ended
        self.hosts = []             # host values per enqueued update, oldest first
        self.hosts_base = 1         # ordinal of self.hosts[0]

    # -- layout -----------------------------------------------------------------------------------------------------------------
    def _flatten(self, aggs, extra):
        """-> (layout, [cell tensors], [host values]) of one update's aggregated logging outputs + optimizer scalars."""
        layout, cells, hosts = [], [], []
        for i, agg in enumerate(aggs):
            def walk(d, keys):
                for k, v in d.items():
                    if isinstance(v, dict):
                        layout.append((i, keys + (k,), "dict", None))
                        walk(v, keys + (k,))
                    elif torch.is_tensor(v) and v.device.type != "cpu":
                        if v.numel() != 1:
                            raise ValueError(f"stats: {cell_path(i, keys + (k,))} is a tensor of {v.numel()} elements; a logged entry is one scalar")
                        if v.dtype not in TYPE_CODES:
                            raise ValueError(f"stats: {cell_path(i, keys + (k,))} has dtype {v.dtype}; st5_stats_record widens "
                                             "fp32, fp64, bf16, fp16, int64, int32, uint8 and bool")
                        if v.device != self.device:
                            raise ValueError(f"stats: {cell_path(i, keys + (k,))} lives on {v.device}, the update runs on {self.device}")
                        layout.append((i, keys + (k,), "cell", v.dtype))
                        cells.append(v)
                    else:
                        if torch.is_tensor(v):
                            if v.numel() != 1:
                                raise ValueError(f"stats: {cell_path(i, keys + (k,))} is a tensor of {v.numel()} elements; a logged entry is one scalar")
                            v = v.item()
                        layout.append((i, keys + (k,), "host", None))
                        hosts.append(v)
            walk(agg, ())
        for name, t in extra:
            layout.append((None, (name,), "cell", t.dtype))
            cells.append(t)
        return layout, cells, hosts

    def _fix(self, layout, cells):
        if len(cells) < 1 or len(cells) > MAX_CELLS:
            raise ValueError(f"stats: {len(cells)} logged device scalars; st5_stats_record takes 1 to {MAX_CELLS}")
        assert not torch.cuda.is_current_stream_capturing(), "the first update of a PretrainUpdate is never the captured pass"
        self.layout = layout
        self.cell_types = [v.dtype for v in cells]
        self.paths = [(cell_path(i, k) if i is not None else "opt." + k[0]) for i, k, kind, _ in layout if kind == "cell"]
        self.n_cells = n = len(cells)
        opt_cells = [e[1][0] for e in layout if e[0] is None]      # (the optimizer's scalars are the last cells, in this order)
        for j, name in enumerate(opt_cells):
            if name == "gnorm_sq":
                self.gnorm_cell = n - len(opt_cells) + j
            elif name == "skipped":
                self.skipped_cell = n - len(opt_cells) + j
        dev = self.device
        self.ring = torch.zeros(self.rows, 1 + n, dtype=torch.int64, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.addr_dev = torch.zeros(n, dtype=torch.int64, device=dev)
        self.types_dev = torch.tensor([TYPE_CODES[t] for t in self.cell_types], dtype=torch.int32).to(dev)
        self.images = [torch.zeros(self.rows, 1 + n, dtype=torch.int64).pin_memory() for _ in range(2)]
        self._addr_host = [torch.zeros(n, dtype=torch.int64).pin_memory() for _ in range(2)]
        self._graph_addr = torch.zeros(n, dtype=torch.int64).pin_memory()

    def _check(self, layout):
        if layout == self.layout:
            return

        def name(e):
            return cell_path(e[0], e[1]) if e[0] is not None else "opt." + e[1][0]
        for a, b in zip(layout, self.layout):
            if a[:2] != b[:2]:
                raise ValueError(f"stats: the logging output changed between updates: {name(a)} where the first update had {name(b)}")
            if a != b:
                raise ValueError(f"stats: {name(a)} changed between updates: {a[2]} {a[3]}, the first update had {b[2]} {b[3]}")
        longer, which = (layout, "new") if len(layout) > len(self.layout) else (self.layout, "missing")
        raise ValueError(f"stats: the logging output changed between updates: {name(longer[min(len(layout), len(self.layout))])} is {which}")

    # -- the update's side ------------------------------------------------------------------------------------------------------
    def record(self, aggs, opt=None):
        """The record launch of one update, on the current stream (the update's own), behind everything that wrote a logged scalar.
        `aggs` hold the logged tensors: the caller keeps them referenced until this returns; under capture they are kept here until
        capture_done()."""
        extra = [("gnorm_sq", opt.gnorm_sq)] if (opt is not None and (self.clip_norm > 0 or self.guard)) else []
        if self.guard:
            from .ddp import GUARD_SKIPPED
            extra.append(("skipped", opt.guard[GUARD_SKIPPED:GUARD_SKIPPED + 1]))     # (a view: the cell's own address)
        layout, cells, hosts = self._flatten(aggs, extra)
        if self.layout is None:
            self._fix(layout, cells)
        else:
            self._check(layout)
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            # the node reads the device column; the capture-time addresses are put there once the capture has ended
            self._graph_addr.copy_(torch.tensor([v.data_ptr() for v in cells], dtype=torch.int64))
            self._graph_hosts = hosts
            self._held = (aggs, cells)
        else:
            s = self._addr_slot
            if self._addr_event[s] is not None:
                self._addr_event[s].synchronize()      # (the upload two eager steps ago: long done)
            self._addr_host[s].copy_(torch.tensor([v.data_ptr() for v in cells], dtype=torch.int64))
            self.addr_dev.copy_(self._addr_host[s], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._addr_event[s] = ev
            self._addr_slot = s ^ 1
            self._dev_is_graph = False
        Fn.stats_record(self.addr_dev, self.types_dev, self.ring, self.counter, self.rows, self.n_cells)
        if not capturing:
            self.hosts.append(hosts)
            self.sched.updated()

    def capture_done(self):
        """Behind the capture, on the update's stream: the captured node's addresses go to the device and the held tensors go."""
        self._held = None
        self._upload_graph_addresses()

    def _upload_graph_addresses(self):
        self.addr_dev.copy_(self._graph_addr, non_blocking=True)     # (a pinned image that is never rewritten)
        self._dev_is_graph = True

    def before_replay(self):
        if not self._dev_is_graph:      # (an eagerly enqueued update since the last replay)
            self._upload_graph_addresses()

    def replayed(self):
        """A replay of the captured update was enqueued on the current stream."""
        self.hosts.append(self._graph_hosts)
        self.sched.updated()

    # -- harvest ----------------------------------------------------------------------------------------------------------------
    def _copy_ring(self, image):
        self.images[image].copy_(self.ring, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def _read_row(self, image, row):
        r = self.images[image][row].numpy().copy()
        return int(r[0]), r[1:]

    def _value(self, cells, j):
        t = self.cell_types[j]
        if t.is_floating_point:
            return float(cells[j:j + 1].view("float64")[0])
        v = int(cells[j])
        return bool(v) if t == torch.bool else v

    def _entries(self, taken):
        out = []
        for k, cells in taken:
            hosts = self.hosts[k - self.hosts_base]
            aggs, ci, hi = [], 0, 0
            for i, keys, kind, _ in self.layout:
                if i is None:
                    continue
                while len(aggs) <= i:
                    aggs.append({})
                node = aggs[i]
                for key in keys[:-1]:
                    node = node[key]
                if kind == "dict":
                    node[keys[-1]] = {}
                elif kind == "cell":
                    node[keys[-1]] = self._value(cells, ci)
                    ci += 1
                else:
                    node[keys[-1]] = hosts[hi]
                    hi += 1
            gsq = self._value(cells, self.gnorm_cell) if self.gnorm_cell is not None else None
            gnorm = math.sqrt(gsq) * self.grad_scale if gsq is not None else None
            out.append({"ordinal": k, "gnorm_sq": gsq, "gnorm": gnorm,
                        "clip": (gnorm > self.clip_norm) if (gnorm is not None and self.clip_norm > 0) else None,
                        **({"skipped": self._value(cells, self.skipped_cell)} if self.skipped_cell is not None else {}),
                        "logging_outputs": aggs})
        if taken:
            last = taken[-1][0]
            del self.hosts[:last + 1 - self.hosts_base]
            self.hosts_base = last + 1
        return out

    def drain(self):
        """(on the update's stream) a final copy of the ring, waited for."""
        if self.layout is not None:
            self.sched.drain()

    def harvest(self):
        return self._entries(self.sched.harvest()) if self.layout is not None else []

    def close(self):
        self._held = None
        self.ring = self.counter = self.images = self.addr_dev = self.types_dev = self._addr_host = self._graph_addr = None
        self._addr_event = [None, None]
        self.hosts = []
