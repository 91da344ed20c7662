"""One optimizer update of the pre-training recipe (`--update-freq 2`: a speech micro-batch and a text micro-batch, SURVEY.md
3.1-3.2) the way bench.py times it: forward + backward of both micro-batches, the gradient exchange over the ranks, global-norm clip
and the fused Adam step -- enqueued eagerly or replayed as a HIP graph.  bench.py and tests/test_bench_update_gpu.py build their step
from THIS class, so the thing that is timed is the thing whose results are checked.

Modes (what the reference's trainer does in turn -- tasks/speecht5.py:519-556 called once per micro-batch by fairseq's
Trainer.train_step, gradients summed, one optimizer step -- is `micro="in_turn"`; the other modes reorder execution, never
arithmetic: every mode produces the SAME bits, tests/test_bench_update_gpu.py and tests/test_replay_long_gpu.py):

  micro      "side_by_side"  (default) both micro-batches on two streams, forward and backward, two gradient buffers summed inside the
                             Adam kernel (a + b == b + a bit for bit).  31.5 ms per update against 39.5 in turn on one MI355X: the
                             two branches fill each other's tile-quantisation tails and launch gaps.  Rounds 3-4 kept this mode off
                             because ~1 % of its replays differed; round 5 found the cause -- one missing `s_waitcnt lgkmcnt(0)` in
                             front of a barrier of the attention backward -- and 300 replayed updates now
                             reproduce the in-turn trajectory bit for bit in every process
             "in_turn"       one stream, one gradient buffer, ddp.accumulate: the reference trainer's order
             "in_turn_2buf"  two streams / two gradient buffers, the second backward ordered behind the first
  graph      True: the update (one rank) or its local phase (several ranks) is captured once and replayed
  several ranks, graph: the captured part is the LOCAL phase (zero_grad, both micro-batches); exchange="phased" (default) cuts it
             into three graphs and all-reduces each completed bucket range under the next one -- with micro="side_by_side" (round 6)
             both micro-batches run inside every phase on two streams and a range is summed over the two gradient buffers before it
             goes out; "one_message": one graph and one all-reduce of the whole buffer behind it; Adam follows eagerly

Data: without a source every update trains on the constructor's `micro_batches` (what bench.py times).  set_source(iterable) makes
every update train on the next element of the iterable -- a list of micro-batches with the signature of the constructor's: replayed,
through one st5_batch_load at the head of the captured step into the constructor's tensors (graph.BatchFeed; they are overwritten);
eagerly, directly on the batch's own tensors (DESIGN.md "Batch feed").

Statistics: stats=True (one rank) ends every update with one st5_stats_record launch -- the last node of the captured step -- that
copies the logged device scalars of every micro-batch and the squared gradient norm into a row of a device ring; logging_outputs()
returns, without waiting, the updates whose ring copy has completed, as the reference trainer's list of train_step outputs
(train_stats.StatsRecorder).  Off by default: nothing is launched, allocated or computed for it.

Non-finite gradients: nonfinite="skip" puts the Adam step behind a verdict on the device (ddp.FusedAdam(skip_nonfinite=True),
st5_adam_step_guard).  An update whose squared gradient norm is NaN, inf or overflowed leaves parameters, both Adam
moments and the bf16 image as they were and zeroes the gradient buffers; the next update trains on.  It works eagerly, recorded and
replayed, in every `micro` mode, with and without a source: in the captured step the guarded launch IS the Adam node, with frozen
arguments and one guard block for the life of the update.  What differs from the reference's trainer, which reads the norm on the host:
  * `n` (fairseq's num_updates) counts ATTEMPTED updates -- the host cannot know a verdict in time without a synchronisation -- so a
    skipped update still advances set_num_updates() and the learning-rate schedule (fairseq leaves num_updates standing).  The
    schedule index is late by the number of skipped updates; Adam's own step count, kept on the device, is exact.
  * a skipped update has still run its forward: buffers a forward updates (the post-net's BatchNorm running statistics) have seen the
    batch, as they have in the reference on an overflowed step.  Nothing tries to undo that.
  * several ranks: the norm is taken over the REDUCED gradient buffer, which holds the same bits on every rank, so every rank reaches
    the same verdict on its own; no verdict is exchanged.
With stats=True every update's entry carries `skipped` (0 / 1), read from the guard block by the same st5_stats_record launch.
nonfinite_limit=k (needs stats=True) is a host policy on the harvested entries: when logging_outputs() or finish() see k consecutive
skipped updates they raise FloatingPointError naming the first of them -- the counterpart of fairseq giving up at its minimum loss
scale, and always late by up to one harvest of the ring (stats_rows // 2 updates), during which further updates were skipped too.
nonfinite=None (default): nothing of this exists; the update is built and launched exactly as before.

ASR fine-tuning (an s2t micro-batch): under a source the criterion must run with sentence_avg=True and, with a CTC term,
device_targets=True (check_s2t_source refuses by option name); the source is collate.SpeechToTextCollater(fixed_shape=...).
TTS fine-tuning (a t2s micro-batch): the source is collate.TextToSpeechCollater(fixed_shape=...), whose batches carry
net_input["tgt_live"] -- the mel post-net then ranges over the frames of the own-length batch (st5_batchnorm_act_*_live) -- and with
stats=True the criterion runs with device_ntokens=True (check_t2s_source refuses by option name).  s2s and s2c stay refused.
Freeze boundaries: --freeze-encoder-updates / --freeze-decoder-updates are host decisions of the forward (`threshold <= num_updates`),
so a captured step has the decision of the update it was captured with.  update() raises RuntimeError, before anything is enqueued or
pulled, when the coming replay's update number lies on the other side of a threshold; recapture=True (needs prefetch_host=False)
instead drops the graph there and runs prepare_graph() again -- that update() call executes two updates, as recording steps -- with
source, statistics and optimizer carrying on; `captures` counts the graphs, `opt.t` the updates.

Save and resume (checkpoint.py): state_dict() / load_state_dict() / snapshot() / save_checkpoint(path) -- everything that
decides the next update's bits, as CPU data in a file that loads with weights_only=True; a resumed run continues bit for bit.  One rank;
a replayed run saves with prefetch_host=False, after at least one replay since the capture; a load comes before prepare_graph().  The
source's position is the caller's: after a load, set_source() gets an iterable positioned `batches_pulled` elements in.  A run that
never calls these methods launches and allocates nothing for them.
"""
import os

import torch
import torch.distributed as dist

from . import functional as Fn


FREEZE_OPTIONS = ("freeze_encoder_updates", "freeze_decoder_updates")


def freeze_thresholds(model):
    """{option: sorted thresholds} over the modules of `model` that decide `threshold <= num_updates` on the host in their forward
    (modules/encoder.py, modules/speech_encoder_prenet.py for --freeze-encoder-updates; the decoder's pre- / post-nets and layers for
    --freeze-decoder-updates).  A captured step has that decision baked in."""
    out = {}
    for m in model.modules():
        for opt in FREEZE_OPTIONS:
            v = getattr(m, opt, None)
            if isinstance(v, (int, float)) and not isinstance(v, bool):
                out.setdefault(opt, set()).add(v)
    return {k: sorted(v) for k, v in out.items()}


def freeze_crossing(thresholds, n_captured, n):
    """The first (option, threshold) whose decision `threshold <= num_updates` differs between update `n_captured` (the update number
    the graph's forward was captured with) and update `n`; None when every module decides as captured."""
    for opt in sorted(thresholds):
        for thr in thresholds[opt]:
            if (thr <= n_captured) != (thr <= n):
                return opt, thr
    return None


def check_s2t_source(micro_batches, criterion, graph=True):
    """An s2t micro-batch under a source of a replayed update (graph.HOST_VALUES_FREE lets its host `ntokens` differ from batch to
    batch): refuse, naming the option, a criterion that puts that host value -- or a host read -- into the captured step."""
    if not graph:
        return
    for i, s in enumerate(micro_batches):
        if s.get("task_name") != "s2t":
            continue
        c = getattr(criterion, "text_criterion", criterion)
        if not getattr(c, "sentence_avg", False):
            raise ValueError(f"micro_batches[{i}] (s2t) under a source needs the criterion's sentence_avg=True: with sentence_avg=False the "
                             "sample's host `ntokens` is the loss divisor, a launch argument of the captured step, and the batch feed "
                             "lets it differ from batch to batch")
        if getattr(c, "ctc_weight", 0) > 0 and not getattr(c, "device_targets", False):
            raise ValueError(f"micro_batches[{i}] (s2t) under a source with ctc_weight > 0 needs the criterion's device_targets=True: "
                             "device_targets=False builds the CTC targets with masked_select, a device-to-host read no capture survives")


def check_t2s_source(micro_batches, criterion, graph=True, stats=False):
    """A t2s micro-batch under a source of a replayed update: refuse, naming the option, a batch without the live step count -- the mel
    post-net's batch statistics and convolutions would range over the fixed shape's padding, another model than the reference's,
    silently -- and, with stats=True, a criterion that logs the sample's host `ntokens` (graph.HOST_VALUES_FREE_T2S lets it differ from
    batch to batch; a replay would report the captured pass's)."""
    if not graph:
        return
    for i, s in enumerate(micro_batches):
        if s.get("task_name") != "t2s":
            continue
        ni = s.get("net_input")
        if not isinstance(ni, dict) or ni.get("tgt_live") is None:
            raise ValueError(f"micro_batches[{i}] (t2s) under a source needs net_input['tgt_live'], the device count of decoder steps "
                             "collate.TextToSpeechCollater(fixed_shape=...) adds: without it the post-net's BatchNorm statistics and "
                             "convolutions take in the frames a fixed shape pads with")
        c = getattr(criterion, "speech_criterion", criterion)
        if stats and not getattr(c, "device_ntokens", False):
            raise ValueError(f"micro_batches[{i}] (t2s) under a source with stats=True needs the criterion's device_ntokens=True: with "
                             "device_ntokens=False the log carries the sample's host `ntokens`, which the batch feed lets differ from "
                             "batch to batch")


class PretrainUpdate:
    def __init__(self, task, model, criterion, micro_batches, *, lr=2e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.01, clip_norm=5.0,
                 graph=True, micro="side_by_side", wgrad_stream=None, prefetch_host=True, device=None, lr_fn=None, exchange="phased", exchange_payload="fp32",
                 stats=False, stats_rows=64, nonfinite=None, nonfinite_limit=None, recapture=False):
        from .ddp import FlatGradDataParallel, FusedAdam
        assert micro in ("side_by_side", "in_turn_2buf", "in_turn")
        self.task, self.model, self.crit, self.micro = task, model, criterion, list(micro_batches)
        self.mode = micro
        self.use_graph = graph
        # recapture=True: a replay that would cross a freeze boundary (--freeze-encoder-updates / --freeze-decoder-updates: host
        # decisions of the forward, baked into the captured step) drops the graph and runs prepare_graph() again instead of raising.
        # The helper thread prepares a replay one step ahead -- its host draws and the pulled batch would belong to a replay that
        # never runs -- so this needs prefetch_host=False
        if recapture and prefetch_host:
            raise ValueError("recapture=True needs prefetch_host=False: under prefetch the next replay's batch is already pulled and its "
                             "host random numbers are drawn when the freeze boundary is met")
        self.recapture = bool(recapture)
        self.captures = 0             # graphs captured so far (prepare_graph() calls that completed)
        self._freeze = freeze_thresholds(model)
        self._graph_n = None          # the update number the captured forward was traced with (= the first replay's)
        self._graph_replays = 0       # replays of the current graph
        self.device = device if device is not None else next(model.parameters()).device
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # (checked before anything is attached to the model)
        if nonfinite not in (None, "skip"):
            raise ValueError(f"nonfinite = {nonfinite!r}: None (no check, the default) or 'skip'")
        if nonfinite_limit is not None:
            if nonfinite != "skip" or not stats:
                raise ValueError("nonfinite_limit is a policy on the harvested statistics of a guarded update: it needs nonfinite='skip' "
                                 "and stats=True")
            if not (isinstance(nonfinite_limit, int) and nonfinite_limit >= 1):
                raise ValueError(f"nonfinite_limit = {nonfinite_limit!r}: a number of consecutive skipped updates, at least 1")
        self.nonfinite_limit = nonfinite_limit
        self._harvested = []          # entries taken out of the ring, not yet handed out by logging_outputs()
        self._skip_run = 0            # consecutive skipped updates at the end of what was harvested so far ...
        self._skip_run_first = None   # ... and the number of the first of them
        # stats=True: every update ends with one st5_stats_record launch (train_stats.StatsRecorder) and
        # logging_outputs() hands the caller what the reference's trainer logs; off, nothing below exists
        self.stats = None
        self._aggs = None         # the aggregated logging outputs of the update being enqueued, in micro-batch order
        self._advanced = []       # (num_updates, lr) per advance(), oldest first: row k of the statistics belongs to the k-th
        self._advanced_base = 1
        if stats:
            if self.world > 1:
                raise ValueError("stats=True with a process group of more than one rank: the logging outputs of several ranks are "
                                 "gathered by the trainer, which this update does not do")
            parts = list(criterion.modules()) if isinstance(criterion, torch.nn.Module) else [criterion]
            if graph and any(getattr(c, "sync_logging", False) for c in parts):     # (SpeechT5Criterion keeps the flag on its four parts)
                raise ValueError("stats=True with graph=True needs a criterion that keeps its logged scalars on the device "
                                 "(sync_logging=False): a `.item()` inside the captured step would fail the capture")
            from .train_stats import StatsRecorder
            self.stats = StatsRecorder(self.device, rows=stats_rows, clip_norm=clip_norm, grad_scale=1.0 / len(self.micro),
                                       **({"guard": True} if nonfinite == "skip" else {}))
        # no weight-gradient stream, no attention helper stream: beside two micro-batch streams they cost time (42.0 against 31.5 ms,
        # profiles/r5_replay_hunt.txt); results are the same bits with and without them
        if wgrad_stream is None:
            wgrad_stream = False
        self.ddp = FlatGradDataParallel(model, wgrad_stream=wgrad_stream)
        self.opt = FusedAdam(self.ddp, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, clip_norm=clip_norm,
                             **({"skip_nonfinite": True} if nonfinite == "skip" else {}))
        self.lr_fn = lr_fn
        self.prefetch_host = prefetch_host
        assert exchange_payload in ("fp32", "bf16")
        # several ranks, one-message exchange: the gradient buffer travels as bf16 (half the link bytes; local sums and Adam stay fp32)
        self.exchange_payload = torch.bfloat16 if exchange_payload == "bf16" else None
        self._payload_asked = exchange_payload
        # several ranks + graph: graph = local phase, eager tail = all-reduce + Adam.  Several ranks WITHOUT a graph and two gradient
        # buffers (micro != "in_turn"): the same split, enqueued eagerly -- the bucket triggers of the eager overlapped path need ONE
        # buffer of summed gradients, so accumulate_overlapped() is only legal inside local_phase() (`--gpus N --no-graph`
        # with the default micro-batch mode used to trip that assert)
        self.split = self.ddp.collectives and (graph or micro != "in_turn")
        # several ranks + graph + one stream: the exchange is OVERLAPPED with the last micro-batch's backward -- the local phase
        # is captured as three graphs cut at bucket boundaries (ddp.cut_points), and after each of them the bucket range it
        # completed goes to the process group as one asynchronous all-reduce (RCCL's stream) while the next graph runs
        # (exchange="one_message": one graph + one all-reduce of the whole buffer afterwards, the round-2 form)
        # (ST5_EAGER_PHASED=1: the same three phases enqueued eagerly -- the tests' reference point)
        # micro="side_by_side" (round 6, the default form): the same phases with BOTH micro-batches inside each of them, on two
        # streams forked from and joined into the phase's graph; a bucket range goes out once both backward passes have completed it
        # and its two gradient buffers are summed (phase_fns_side_by_side)
        self.phased = ((self.split or (self.ddp.collectives and os.environ.get("ST5_EAGER_PHASED") == "1"))
                       and micro in ("in_turn", "side_by_side") and exchange == "phased" and len(self.micro) >= 1
                       and (micro == "in_turn" or len(self.micro) == 2))
        if self.phased and not self.ddp.overlap_exchange:    # (decided once per group in FlatGradDataParallel, the same on every rank)
            self.phased = False      # one message behind the local phase: no collective beside the backward's kernels
        if self.exchange_payload is not None and (self.phased or not self.split):
            # (the bf16 payload exists for the one-message exchange only; silently exchanging fp32 is not what was asked)
            import warnings
            warnings.warn("speecht5_amd: exchange_payload='bf16' applies to the one-message exchange only (exchange='one_message' with a "
                          "replayed or split update); this update exchanges fp32 gradients "
                          f"({'phased' if self.phased else 'bucketed, eager'} form)")
            self.exchange_payload = None
        self._ph = None
        self.n = 0            # update counter (fairseq's num_updates)
        self.sg = None
        self.feed = None      # graph.BatchFeed once set_source() was called
        # checkpoint.py: batches pulled before a loaded checkpoint was saved; the snapshot in flight; its device shadow (allocated by
        # the first snapshot(), never freed while the update lives).  Nothing of it exists for a run that never saves.
        self._pulled_base = 0
        self._snapshot = None
        self._shadow = None
        # Every update is enqueued on a stream of its own, never on the legacy NULL stream: on this runtime (ROCm 7.2) work issued
        # to the NULL stream from two host threads (the forward from the caller's thread, the backward from autograd's worker
        # thread) is NOT kept in issue order once another stream is busy -- measured: with the speech micro-batch on the NULL
        # stream and the text micro-batch beside it, the reduction kernel of conv layer 0's backward read partials its
        # predecessor in the same stream had not written yet (round 3, docs/HISTORY.md 4a: NaN-poisoned partials came through in 4 of 4
        # updates; 0 of 4 on an explicit stream).
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None

    # -- pieces ---------------------------------------------------------------------------------------------------------
    def _fwd(self, s):
        if self.stats is None:
            return self.task.forward_loss(s, self.model, self.crit, self.n)
        loss, agg = self.task.forward_loss(s, self.model, self.crit, self.n, return_log=True)
        self._aggs.append(agg)
        return loss

    def local_part(self):
        """(several ranks, graph) what the graph holds: gradients of this rank's micro-batches, summed into ddp.flat."""
        self.ddp.zero_grad()
        with self.ddp.local_phase():
            if self.mode == "in_turn":
                self.ddp.accumulate(self.micro, lambda s: self.task.train_step(s, self.model, self.crit, None, self.n, sync=False))
            else:
                self.ddp.accumulate_overlapped(self.micro, self._fwd, backward="in_turn" if self.mode == "in_turn_2buf" else "side_by_side")
        self.ddp.sum_gradient_buffers()
        # the deferred reductions (split-K slabs, LayerNorm partials) are folded INSIDE the captured part: their descriptors are
        # host state of the library, consumed by the first flush -- left to the eager tail, the first replay's tail would fold
        # them and every later replay's slabs would never reach the gradient buffer
        self.ddp.flush_deferred()

    # -- phased local part (several ranks, overlapped exchange) ------------------------------------------------------------
    def cut_buckets(self):
        """Where the backward is cut: behind the decoder (+ both heads, the shared cross-attention K/V projection: ~60 M parameters
        complete) and inside the encoder stack -- at the input of layer L/3 (Base: layer 4), so that the LAST message, the one nothing
        is left to hide, is the smallest: 234 / 227 / 156 MB for Base (round 5 cut at L/2: 234 / 170 / 213 MB).  ST5_ENC_CUT=<layer>
        moves the second cut (A/B)."""
        mb = self.ddp.module_bucket
        enc = getattr(self.model, "encoder", None)
        cuts = []
        if enc is not None:
            if (id(enc), "out") in mb:
                cuts.append(mb[(id(enc), "out")])
            layers = list(getattr(enc, "layers", []))
            at = int(os.environ.get("ST5_ENC_CUT", len(layers) // 3))
            if len(layers) >= 4 and 0 < at < len(layers) and (id(layers[at]), None) in mb:
                cuts.append(mb[(id(layers[at]), None)])
        return sorted(set(cuts))

    def phase_fns(self):
        """The local phase as len(cuts) + 1 callables and, behind each, the hand-over of a bucket range to the process group.
        The bucket ranges are STATIC (cut_buckets() is a function of the model alone, the same list on every rank): message k
        covers the buckets up to cuts[k], the last one the rest.  What this rank's forward materialised only decides how many of
        its own backward phases run inside nominal phase k (a cut whose input needed no gradient on this rank does not
        materialise: the phase in front of it then runs through, and the nominal phase behind it is empty) -- the number and the
        extent of the collectives never depend on per-rank state."""
        ddp, cuts_b = self.ddp, self.cut_buckets()
        nph = len(cuts_b) + 1
        nb = len(ddp.buckets)

        def run_until(b):     # this rank's backward phases until bucket b (None: every bucket) is complete
            while self._ph_done < len(self._ph) and (b is None or self._ph_complete < b):
                fn, upto = self._ph[self._ph_done]
                with ddp.local_phase():
                    fn()
                self._ph_complete = nb - 1 if upto is None else upto
                self._ph_done += 1

        def first():
            ddp.zero_grad()
            with ddp.local_phase():
                for mb in self.micro[:-1]:
                    self.task.train_step(mb, self.model, self.crit, None, self.n, sync=False)
                with ddp.cut_points(cuts_b) as cuts:
                    loss = self._fwd(self.micro[-1])
                self._ph = ddp.backward_phases(loss, cuts)
            self._ph_done, self._ph_complete = 0, -1
            fn, upto = self._ph[0]           # (from the loss to the last materialised cut: always runs here)
            with ddp.local_phase():
                fn()
            self._ph_complete = nb - 1 if upto is None else upto
            self._ph_done = 1
            run_until(cuts_b[0] if cuts_b else None)
            ddp.flush_deferred()

        def later(k):
            def fn():
                run_until(cuts_b[k] if k < len(cuts_b) else None)
                ddp.flush_deferred()
            return fn

        def reduce_after(k):
            def fn():
                ddp.reduce_bucket_range(cuts_b[k] if k < len(cuts_b) else None)
            return fn
        return [first] + [later(k) for k in range(1, nph)], [reduce_after(k) for k in range(nph)]

    def phase_fns_side_by_side(self):
        """phase_fns() for the two micro-batches SIDE BY SIDE: every phase forks the second micro-batch's stream from the phase's own
        and joins it again, so each phase is one graph with two branches (the form the one-graph local phase already has); both
        forward passes run under cut_points() and keep their own list of backward phases; nominal phase k runs each micro-batch's
        backward, on its stream and into its gradient buffer, until bucket cuts[k] is complete in BOTH, folds each stream's deferred
        reductions, joins, sums the two buffers over the completed bucket range (ddp.sum_bucket_range: flat += flat2, fp32, the sum the
        pair kernels of the one-rank optimizer step form) -- and the caller hands that range of `flat` to the process group while the
        next phase's graph runs.  Bucket ranges are static (see phase_fns)."""
        import torch
        ddp, cuts_b = self.ddp, self.cut_buckets()
        nph = len(cuts_b) + 1
        nb = len(ddp.buckets)
        st = {}

        def streams():
            cur = ddp.pair_streams(2)           # (forks the second stream from the current one)
            return cur, [cur, ddp._fwd_streams[0]]

        def run_until(i, b):                    # micro-batch i's backward phases until bucket b (None: every bucket) is complete
            ph = st["ph"][i]
            while st["done"][i] < len(ph) and (b is None or st["complete"][i] < b):
                fn, upto = ph[st["done"][i]]
                fn()
                st["complete"][i] = nb - 1 if upto is None else upto
                st["done"][i] += 1

        def backward_to(k, first=False, forked=None):
            cur, ss = forked if forked is not None else streams()
            for i in (0, 1):
                with ddp._grad_slot(i), torch.cuda.stream(ss[i]), ddp.local_phase():
                    if first:
                        fn, upto = st["ph"][i][0]      # (from the loss to the last materialised cut: always runs here)
                        fn()
                        st["complete"][i] = nb - 1 if upto is None else upto
                        st["done"][i] = 1
                    run_until(i, cuts_b[k] if k < len(cuts_b) else None)
                    ddp.flush_stream_deferred()
            cur.wait_stream(ss[1])
            ddp.sum_bucket_range(cuts_b[k] if k < len(cuts_b) else None)

        def first():
            ddp.zero_grad()
            cur, ss = streams()
            st["ph"], st["done"], st["complete"] = [None, None], [0, 0], [-1, -1]
            with ddp.local_phase():
                for i, mb in enumerate(self.micro):
                    with torch.cuda.stream(ss[i]), ddp.cut_points(cuts_b) as cuts:
                        loss = self._fwd(mb)
                    st["ph"][i] = ddp.backward_phases(loss, cuts)
            backward_to(0, first=True, forked=(cur, ss))     # (no join between forward and backward: each chain runs on)

        def later(k):
            def fn():
                backward_to(k)
                if k == nph - 1:
                    st["ph"] = None             # (the autograd graphs of this update may go)
            return fn

        defer = os.environ.get("ST5_PHASED_DEFER_EXCHANGE") == "1"    # (diagnostic: the same three graphs, ONE message behind the last)

        def reduce_after(k):
            def fn():
                if defer and k < nph - 1:
                    return
                ddp.reduce_bucket_range(cuts_b[k] if (k < len(cuts_b) and not defer) else None)
            return fn
        self._ph_sbs = st
        return [first] + [later(k) for k in range(1, nph)], [reduce_after(k) for k in range(nph)]

    def finish_exchange_and_update(self):
        self.ddp.check_grad_views()
        self.ddp.wait_reductions()
        self.opt.step(grad_scale=1.0 / (len(self.micro) * self.world))

    def exchange_and_update(self):
        """(several ranks, graph) eager tail: sum over ranks, then mean over ranks and micro-batches inside Adam."""
        self.ddp.all_reduce_gradients(average=False, payload=self.exchange_payload)
        self.opt.step(grad_scale=1.0 / (len(self.micro) * self.world))

    def step(self):
        """One update enqueued on the current stream (no host synchronisation)."""
        if self.phased:
            for fn, bt in zip(*(self.phase_fns() if self.mode == "in_turn" else self.phase_fns_side_by_side())):
                fn()
                bt()
            self.finish_exchange_and_update()
            return
        if self.split:
            self.local_part()
            self.exchange_and_update()
            return
        ddp = self.ddp
        ddp.zero_grad()
        self._aggs = [] if self.stats is not None else None
        if self.mode == "in_turn":
            # --update-freq 2: gradients of the first micro-batch only accumulate (no_sync); the bucket all-reduces are launched
            # from the backward of the LAST micro-batch, each bucket once, after its last local contribution
            outs = ddp.accumulate(self.micro, lambda s: self.task.train_step(s, self.model, self.crit, None, self.n, sync=False))
            if self.stats is not None:
                self._aggs = [o[2] for o in outs]
        else:
            ddp.accumulate_overlapped(self.micro, self._fwd, backward="in_turn" if self.mode == "in_turn_2buf" else "side_by_side")
        ddp.finish()
        self.opt.step(grad_scale=1.0 / len(self.micro))
        if self.stats is not None:
            # the last launch of the update, on its own stream behind Adam (side by side: behind the join of the second stream, so
            # behind every kernel that wrote a logged scalar); self._aggs holds the logged tensors until it is enqueued
            try:
                self.stats.record(self._aggs, self.opt)
            finally:
                self._aggs = None

    def advance(self):
        """Host-side state a replayed step does not touch: the update counter (quantizer temperature, freeze counters), lr."""
        self.n += 1
        self.model.set_num_updates(self.n)
        if self.lr_fn is not None:
            self.opt.lr = self.lr_fn(self.n)
        if self.stats is not None:
            self._advanced.append((self.n, float(self.opt.lr)))

    # -- driving --------------------------------------------------------------------------------------------------------
    def set_source(self, iterable):
        """Every following update trains on the next element of `iterable`: a list of micro-batches with the signature (key paths,
        shape and dtype per tensor leaf, task_name) of the constructor's.  The update pulls from it itself, on the calling thread,
        one element per update (the two recording steps and the capture of prepare_graph() one each), always before that step's host
        random draws; a batch the recorded step cannot take is refused with a ValueError naming the path.  When the source ends,
        the update already prepared still runs and the following update() raises StopIteration.  For a replayed update call this
        BEFORE prepare_graph(): the batch load is the first node of the captured step.  A later call swaps the iterable (next epoch)."""
        from .graph import BatchFeed
        if self.sg is not None and self.sg.feed is None:
            raise RuntimeError("set_source() after prepare_graph(): the batch load is the first node of the captured step and this "
                               "graph was captured without it")
        check_s2t_source(self.micro, self.crit, graph=self.use_graph)
        check_t2s_source(self.micro, self.crit, graph=self.use_graph, stats=self.stats is not None)
        if self.feed is None:
            self.feed = BatchFeed(self.micro, self.device)
        self.feed.set_source(iterable)
        if self.sg is not None:
            self.sg.sched.new_source()

    def eager_update(self):
        if self.feed is not None:
            # one batch of the source, run as it is: the step reads the batch's own tensors (no copy, no static input)
            rec = self.feed.pull(for_eager=True)
            static, self.micro = self.micro, list(rec.batch)
            try:
                self._eager_update()
            finally:
                self.micro = static
            return
        self._eager_update()

    def _eager_update(self):
        self.advance()
        if self.stream is None:
            self.step()
            return
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            self.step()
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def prepare_graph(self):
        """Two recording updates + capture (three updates' worth of host random draws; two of them executed)."""
        from .graph import StepGraph
        # the two recording steps and the captured pass run as updates n + 1, n + 2, n + 3: every module must take the same freeze
        # decision in all three, or the captured step is not the recorded one
        hit = freeze_crossing(self._freeze, self.n + 1, self.n + 3) or freeze_crossing(self._freeze, self.n + 2, self.n + 3)
        if hit is not None:
            raise RuntimeError(f"prepare_graph() at update {self.n + 1}: {hit[0]} = {hit[1]} lies inside the two recording steps and the "
                               f"captured pass (updates {self.n + 1} to {self.n + 3}); run eager updates up to the boundary first")
        if self.feed is not None:
            check_s2t_source(self.micro, self.crit)
            check_t2s_source(self.micro, self.crit, stats=self.stats is not None)
        if self.phased:
            phases, between = self.phase_fns() if self.mode == "in_turn" else self.phase_fns_side_by_side()
            self.sg = StepGraph(None, opt=self.opt, model=self.model, device=self.device, on_step=self.advance,
                                prefetch_host=self.prefetch_host, after_fn=self.finish_exchange_and_update, stream=self.stream,
                                phases=phases, between=between, feed=self.feed)
        else:
            self.sg = StepGraph(self.local_part if self.split else self.step, opt=self.opt, model=self.model, device=self.device,
                                on_step=self.advance, prefetch_host=self.prefetch_host,
                                after_fn=self.exchange_and_update if self.split else None, stream=self.stream, feed=self.feed)
        if self.stats is not None and self.feed is not None:
            from .graph import host_values_free
            from .train_stats import check_feed_host_values, device_logged
            names = [s.get("task_name") for s in self.micro]
            check_feed_host_values(names, host_values_free(), {n: device_logged(n, self.crit) for n in set(names) if device_logged(n, self.crit)})
        self.sg.record()
        self.sg.record()
        self.sg.capture()
        self.captures += 1
        self._graph_n, self._graph_replays = self.n, 0     # (capture() primed the first replay: advance() has counted it)
        if self.stats is not None:
            with torch.cuda.stream(self.sg.stream):
                self.stats.capture_done()     # (the captured record node's source addresses, uploaded once: constant over replays)
        return self.sg

    def _release_graph(self):
        """Drop the captured graph: break the cycle update -> graph -> bound step function -> update (a HIP graph object must not wait
        for the cyclic collector: a collection during a LATER capture destroys it mid-capture)."""
        if self.sg is not None:
            self.sg.step_fn = self.sg.after_fn = self.sg.on_step = self.sg.phases = self.sg.between = None
            self.sg.graph = self.sg.graphs = None
            self._ph = None
            self._ph_sbs = None
            self.sg = None

    def _check_freeze(self):
        """In front of a replay, before anything is enqueued or pulled: does update `n` decide its freezes as the captured step does?
        Returns True when the graph was dropped and captured again (recapture=True: two updates ran, as recording steps)."""
        n = self._graph_n + self._graph_replays
        hit = freeze_crossing(self._freeze, self._graph_n, n)
        if hit is None:
            return False
        if not self.recapture:
            raise RuntimeError(f"{hit[0]} = {hit[1]}: the graph was captured at update {self._graph_n} and update {n} lies on the other "
                               "side of the boundary -- the replay would run the captured freeze decision.  Capture again from here "
                               "(PretrainUpdate(recapture=True, prefetch_host=False) does), or run eagerly")
        # the replays enqueued so far finish before their graph goes (its pool holds their buffers); the host side -- update counter,
        # random streams, source -- stands where an eager loop has it after update n - 1: prepare_graph() carries on from there
        self.sg.drain()
        self.sg.stream.synchronize()
        self._release_graph()
        self.prepare_graph()
        return True

    def update(self):
        """The next update: a replay when a graph exists, else eager."""
        if self.sg is not None:
            if self.feed is not None:      # (the source runs on the caller's stream; the replay waits for an event behind it)
                self.feed.caller_stream = torch.cuda.current_stream(self.device)
            if self._freeze and self._check_freeze():
                return                     # (recapture=True: this call ran the two recording updates of the new graph instead of a replay)
            with torch.cuda.stream(self.sg.stream):
                if self.stats is not None:
                    self.stats.before_replay()
                self.sg.replay()
                self._graph_replays += 1
                if self.stats is not None:
                    self.stats.replayed()     # (host bookkeeping; every stats_rows // 2 updates one asynchronous copy of the ring)
        else:
            self.eager_update()

    def logging_outputs(self, wait=False):
        """(stats=True) the updates harvested since the last call, in order, one entry per update: {"num_updates", "lr", "gnorm_sq",
        "gnorm" (sqrt(gnorm_sq) * grad_scale in fp64: what the clip compared), "clip", "logging_outputs": [agg per micro-batch, as
        train_step(sync=True) returns it]} -- SpeechT5Criterion.reduce_metrics(entry["logging_outputs"]) takes it as it takes the
        reference trainer's list.  wait=False never waits for the device: only rows whose copy has completed are returned.  wait=True
        enqueues a final copy of the ring and waits for it.  nonfinite="skip": every entry also carries "skipped" (0 / 1), and
        "gnorm" is reported with clip_norm == 0 too (of a skipped update it is inf or NaN).  nonfinite_limit=k: raises
        FloatingPointError once the harvested entries end in k or more consecutive skipped updates (the entries are kept: a caller
        that catches the error gets them from the next call)."""
        if self.stats is None:
            raise RuntimeError("logging_outputs(): this update was built with stats=False")
        if wait:
            self._drain_stats()
        self._take_harvest()
        out, self._harvested = self._harvested, []
        return out

    def _take_harvest(self):
        """The rows whose ring copy has completed -> entries kept for the next logging_outputs(); nonfinite_limit is checked on every
        entry once, here, after the entries are safe (a caller that catches the error still gets them from logging_outputs())."""
        got = self.stats.harvest()
        new = []
        for e in got:
            k = e.pop("ordinal")
            n, lr = self._advanced[k - self._advanced_base]
            new.append({"num_updates": n, "lr": lr, **e})
        if got:
            del self._advanced[:k + 1 - self._advanced_base]
            self._advanced_base = k + 1
        self._harvested += new
        if self.nonfinite_limit is not None:
            hit = None
            for e in new:
                if not e["skipped"]:
                    self._skip_run = 0
                    continue
                if self._skip_run == 0:
                    self._skip_run_first = e["num_updates"]
                self._skip_run += 1
                if self._skip_run == self.nonfinite_limit and hit is None:
                    hit = self._skip_run_first
            if hit is not None:
                raise FloatingPointError(f"gradients are Nan/Inf: {self.nonfinite_limit} consecutive updates were skipped, the first of "
                                         f"them update {hit} (nonfinite_limit = {self.nonfinite_limit})")

    def _drain_stats(self):
        """One more copy of the ring on the update's stream, behind the newest update, and a wait for it."""
        if self.stream is not None:
            with torch.cuda.stream(self.stream):
                self.stats.drain()
        else:
            self.stats.drain()

    def finish(self):
        self._finish()
        if self.nonfinite_limit is not None:
            self._take_harvest()     # (the policy sees the end of the run too; the entries stay for logging_outputs())

    def _finish(self):
        if self.sg is not None:
            self.sg.drain()
            torch.cuda.current_stream(self.device).wait_stream(self.sg.stream)
        if self.stats is not None:
            self._drain_stats()      # (everything enqueued so far becomes available to the next logging_outputs())

    def close(self):
        self._finish()               # (no policy check here: close() releases, it does not report)
        if self.feed is not None:
            self.feed.held = []      # (finish() ordered the caller's stream behind the last replay that read them)
        self.ddp.close()
        if self.stats is not None:
            self.stats.close()
        self._release_graph()

    def state(self):
        torch.cuda.synchronize(self.device)
        return self.opt.pflat.clone(), self.opt.m.clone(), self.opt.v.clone(), self.opt.t

    # -- save and resume (checkpoint.py) ---------------------------------------------------------------------------
    @property
    def batches_pulled(self):
        """Batches taken from the source since the start of the run, over every save and load."""
        return self._pulled_base + (self.feed.pulls if self.feed is not None else 0)

    def state_dict(self):
        """Everything that decides the bits of the next update, as CPU data (checkpoint.py has the contents): {"model" (the
        reference's key names), "optimizer", "extra_state", "digest"}.  Synchronous: waits for the update's stream; allocates no device
        memory.  Legal where the host side stands where an eager loop has it after update n: after any eager update, and after a
        replay of a graph built with prefetch_host=False once at least one replay has run since the capture (prepare_graph() stages
        the first replay's batch and host draws).  Elsewhere it raises, naming the condition; so do snapshot() and save_checkpoint().
        Statistics are not part of the state: take logging_outputs(wait=True) first."""
        from . import checkpoint
        return checkpoint.state_dict(self)

    def load_state_dict(self, sd):
        """Restore a state_dict() (checkpoint.load_checkpoint(path) returns one, digests checked) into this update, which must have
        no captured graph: load before prepare_graph().  Parameters and moments are matched by name and written INTO the existing flat
        buffers (every view the model holds stays valid); a missing, extra or differently shaped parameter and a saved hyper-parameter
        that differs from the constructor's are refused with a ValueError naming it.  The bf16 image, the transposed copies and the
        fp8 images are rebuilt, and the rebuilt bf16 image must have the saved digest.  The source is the caller's: after a load give
        set_source() an iterable positioned `batches_pulled` (sd["extra_state"]["batches_pulled"]) elements in."""
        from . import checkpoint
        checkpoint.load_state_dict(self, sd)

    def snapshot(self):
        """state_dict() without stopping training: behind the newest update, on the update's stream, one st5_batch_load copies every
        device segment of the state into a device shadow and one st5_state_digest digests the shadow; a side stream copies shadow and
        digests into pinned memory.  Returns a handle at once -- done() never waits, result() waits for the copy, checks every host
        segment against the device's digest (ValueError naming the segment) and returns the dictionary.  The next update may run as
        soon as this returns.  One snapshot may be in flight: a second call before the first handle's result() raises."""
        from . import checkpoint
        return checkpoint.snapshot(self)

    def save_checkpoint(self, path):
        """snapshot().result() written to `path` through a temporary file in the same directory, fsync and os.replace."""
        from . import checkpoint
        checkpoint.save_checkpoint(self, path)
