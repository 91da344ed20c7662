"""Save and resume training: the state of an update (update.PretrainUpdate), collected and restored in ONE place, verified by a digest
on its way from the device to a file and back.

What decides the bits of update n + 1, and where it lives in the dictionary state_dict() / snapshot().result() return:
  "model"        model.state_dict(), the reference's key names: the fp32 master of every trained parameter (views of the flat buffer
                 `opt.pflat`) and every other tensor of the model (buffers -- the post-net's BatchNorm running statistics -- and
                 parameters outside the flat buffer)
  "optimizer"    both Adam moments as flat fp32 tensors, the layout [(parameter name, offset, numel)] of the flat buffers, the step
                 count `t`, lr, betas, eps, weight decay, clip norm and -- nonfinite="skip" -- the four cells of the guard block
  "extra_state"  num_updates, the dropout seed and counter (functional._S), numpy's global generator, torch's CPU generator, torch's
                 DEVICE generator (the Gumbel noise of the quantizer is drawn from it: modules/gumbel_vector_quantizer.py), the number
                 of batches the feed has pulled, the number of captured graphs, the skip-run bookkeeping of nonfinite_limit
  "digest"       {segment name: 64-bit digest as an int}: "pflat", "m", "v", "guard", "model.<key>" for every tensor of the model
                 outside the flat buffer, and "wflat" -- the bf16 image the Adam kernel wrote, which is NOT saved: load_state_dict()
                 rebuilds it and compares
Not state: the gradient buffers (zero between updates), the transposed and fp8 images (rebuilt from the bf16 image by the code that
refreshes them after every step), the statistics ring (the caller takes logging_outputs(wait=True) first), the data source.

Values are tensors, ints, floats, strings, lists and dicts only: the file loads with torch.load(..., weights_only=True).

The digest (csrc/state_digest_index.h; on the device st5_state_digest): for a segment of n bytes with little-endian 8-byte words w_i
(the last one zero-padded), all arithmetic mod 2^64,
    digest = h((sum_i h(w_i + (i + 1) * 0x9E3779B97F4A7C15)) + n),   h = the splitmix64 finaliser.
host_digest() below is its numpy form."""
import os

import numpy as np
import torch

from . import functional as Fn

FORMAT = 1
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_BLOCK = 1 << 20      # words digested per numpy pass (bounds the temporaries)


# ---------------------------------------------------------------------------------------------------------------------------------
# the digest on the host
# ---------------------------------------------------------------------------------------------------------------------------------
def _mix(x):
    x = x ^ (x >> np.uint64(30))
    x = x * _M1
    x = x ^ (x >> np.uint64(27))
    x = x * _M2
    return x ^ (x >> np.uint64(31))


def _bytes_of(x):
    if torch.is_tensor(x):
        if x.device.type != "cpu":
            raise ValueError("host_digest() reads host memory")
        x = x.detach().contiguous().reshape(-1).view(torch.uint8).numpy()
    elif isinstance(x, (bytes, bytearray, memoryview)):
        x = np.frombuffer(x, dtype=np.uint8)
    else:
        x = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    return x


def host_digest(x):
    """The digest of the bytes of `x` (a CPU tensor of any dtype, a numpy array or a bytes-like object) as a Python int."""
    b = _bytes_of(x)
    n = int(b.size)
    total = np.zeros(1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        whole = n // 8
        for lo in range(0, whole, _BLOCK):
            hi = min(whole, lo + _BLOCK)
            w = b[8 * lo:8 * hi].view("<u8").astype(np.uint64, copy=False)
            pos = np.arange(lo + 1, hi + 1, dtype=np.uint64) * _GOLDEN
            total += _mix(w + pos).sum(dtype=np.uint64)
        if n % 8:
            tail = np.zeros(8, dtype=np.uint8)
            tail[:n % 8] = b[8 * whole:]
            total += _mix(tail.view("<u8").astype(np.uint64) + np.uint64(whole + 1) * _GOLDEN)
        return int(_mix(total + np.uint64(n))[0])


def _cell(v):
    """A digest as the signed 64-bit int a tensor cell (and a checkpoint file) holds <-> as the unsigned value."""
    return int(v) & 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------------
# host generators
# ---------------------------------------------------------------------------------------------------------------------------------
def numpy_state():
    """numpy's global generator as {"keys": int64 tensor of the 624 key words, "pos", "has_gauss", "cached_gaussian"}."""
    name, keys, pos, has_gauss, cached = np.random.get_state()
    if name != "MT19937":
        raise RuntimeError(f"numpy's global generator is {name}, not MT19937")
    return {"keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos), "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}


def set_numpy_state(s):
    np.random.set_state(("MT19937", s["keys"].numpy().astype(np.uint32), int(s["pos"]), int(s["has_gauss"]), float(s["cached_gaussian"])))


def host_state(device=None):
    """The host-side random state of an update: the dropout seed counter, numpy's global stream, torch's CPU generator and, on a
    GPU, torch's device generator (seed and offset: host bookkeeping, read without a synchronisation)."""
    out = {"seed": int(Fn._S.seed), "counter": int(Fn._S.counter), "numpy": numpy_state(), "torch_cpu": torch.get_rng_state().clone()}
    if device is not None and torch.device(device).type == "cuda":
        out["torch_device"] = torch.cuda.get_rng_state(device).clone()
    return out


def set_host_state(s, device=None):
    Fn._S.seed, Fn._S.counter = int(s["seed"]), int(s["counter"])
    set_numpy_state(s["numpy"])
    torch.set_rng_state(s["torch_cpu"].clone())
    if "torch_device" in s and device is not None and torch.device(device).type == "cuda":
        torch.cuda.set_rng_state(s["torch_device"].clone(), device)


# ---------------------------------------------------------------------------------------------------------------------------------
# the optimizer's part (ddp.FusedAdam.state_dict / load_state_dict delegate here)
# ---------------------------------------------------------------------------------------------------------------------------------
def param_names(model):
    return {id(p): name for name, p in model.named_parameters()}


def optimizer_layout(opt):
    names = param_names(opt.ddp.model)
    return [[names[id(p)], int(off), int(p.numel())] for p, off in zip(opt.ddp.params, opt.ddp.offsets)]


def optimizer_meta(opt):
    """Everything of the optimizer's state that lives on the host."""
    return {"layout": optimizer_layout(opt), "numel": int(opt.pflat.numel()), "t": int(opt.t), "lr": float(opt.lr),
            "betas": [float(opt.betas[0]), float(opt.betas[1])], "eps": float(opt.eps), "weight_decay": float(opt.wd),
            "clip_norm": float(opt.clip)}


def optimizer_state_dict(opt):
    """FusedAdam.state_dict(): synchronous, CPU data only."""
    if opt.pflat.is_cuda:
        torch.cuda.synchronize(opt.pflat.device)
    sd = optimizer_meta(opt)
    sd["m"], sd["v"] = opt.m.cpu(), opt.v.cpu()
    if opt.guard is not None:
        sd["guard"] = [int(c) for c in opt.guard.tolist()]
    return sd


def _check_hyper(opt, sd, lr_scheduled=False):
    mine = optimizer_meta(opt)
    for k in ("betas", "eps", "weight_decay", "clip_norm") + (() if lr_scheduled else ("lr",)):
        a, b = sd[k], mine[k]
        if (list(a) != list(b)) if k == "betas" else (float(a) != float(b)):
            raise ValueError(f"checkpoint: {k} = {a!r} was saved, this optimizer was built with {k} = {b!r}")
    if ("guard" in sd) != (opt.guard is not None):
        raise ValueError("checkpoint: the guard block of nonfinite='skip' " + ("was saved, this optimizer has none"
                         if "guard" in sd else "was not saved, this optimizer has one") + " (skip_nonfinite differs)")


def _match_layout(opt, sd):
    """{name: (saved offset, own offset, numel)}; ValueError naming a missing, extra or differently sized parameter."""
    saved = {name: (int(off), int(n)) for name, off, n in sd["layout"]}
    own = {name: (int(off), int(n)) for name, off, n in optimizer_layout(opt)}
    for name in own:
        if name not in saved:
            raise ValueError(f"checkpoint: parameter {name} of this model is missing from the saved layout")
    for name in saved:
        if name not in own:
            raise ValueError(f"checkpoint: the saved layout has parameter {name}, which this model does not have")
    for name, (off, n) in own.items():
        if saved[name][1] != n:
            raise ValueError(f"checkpoint: parameter {name} has {n} elements, the saved layout has {saved[name][1]}")
    for name, (off, n) in saved.items():
        if off < 0 or off + n > int(sd["numel"]) or sd["m"].numel() != int(sd["numel"]) or sd["v"].numel() != int(sd["numel"]):
            raise ValueError(f"checkpoint: parameter {name} lies outside the saved flat buffers")
    return {name: (saved[name][0], off, n) for name, (off, n) in own.items()}


def load_optimizer_state_dict(opt, sd, params=None, lr_scheduled=False):
    """FusedAdam.load_state_dict(): moments, guard block and step count written INTO the existing buffers, matched by parameter name;
    `params` {name: tensor} (the checkpoint's "model" entry) also restores the fp32 master.  The derived images are the caller's
    (rebuild_images)."""
    _check_hyper(opt, sd, lr_scheduled)
    match = _match_layout(opt, sd)
    shapes = {name: tuple(p.shape) for name, p in opt.ddp.model.named_parameters()}
    if params is not None:
        for name in match:
            if name not in params:
                raise ValueError(f"checkpoint: parameter {name} is missing from the saved model")
            if tuple(params[name].shape) != shapes[name]:
                raise ValueError(f"checkpoint: parameter {name} has shape {shapes[name]}, the saved model has {tuple(params[name].shape)}")
    dev = opt.pflat.device
    same = all(s == o for s, o, _ in match.values()) and int(sd["numel"]) == opt.pflat.numel()
    with torch.no_grad():
        if same:
            opt.m.copy_(sd["m"].to(dev))
            opt.v.copy_(sd["v"].to(dev))
        else:
            m, v = sd["m"].to(dev), sd["v"].to(dev)
            opt.m.zero_()
            opt.v.zero_()
            for s, o, n in match.values():
                opt.m[o:o + n].copy_(m[s:s + n])
                opt.v[o:o + n].copy_(v[s:s + n])
        if params is not None:
            for name, (_, o, n) in match.items():
                opt.pflat[o:o + n].copy_(params[name].reshape(-1).to(device=dev, dtype=torch.float32))
        if opt.guard is not None:
            opt.guard.copy_(torch.tensor([int(c) for c in sd["guard"]], dtype=torch.int32).to(dev))
    opt.t = int(sd["t"])
    if not lr_scheduled:
        opt.lr = float(sd["lr"])


def rebuild_images(opt):
    """Every image derived from the fp32 master, by the code that builds it after an optimizer step: the bf16 image (the cast kernel
    of the library: the Adam kernel's rounding), the transposed copies, the fp8 mirror when enabled."""
    Fn.weight_cache.clear()
    if opt.mirror is None:
        return
    Fn._cast_into(opt.pflat.view(1, -1), opt.wflat.view(1, -1))
    for p in opt.ddp.params:
        p._st5_mver = p._version
    Fn.refresh_weight_images()


# ---------------------------------------------------------------------------------------------------------------------------------
# the update's state
# ---------------------------------------------------------------------------------------------------------------------------------
def model_index(upd):
    """[(key of model.state_dict(), name of the flat parameter behind it or None, live tensor)]"""
    names = param_names(upd.model)
    flat = {id(p) for p in upd.opt.ddp.params}
    out = []
    for key, t in upd.model.state_dict(keep_vars=True).items():
        out.append((key, names[id(t)] if id(t) in flat else None, t))
    return out


def device_segments(upd):
    """[(segment name, live tensor)]: everything of the state that lives in device memory, in shadow order."""
    opt = upd.opt
    segs = [("pflat", opt.pflat), ("m", opt.m), ("v", opt.v)]
    if opt.guard is not None:
        segs.append(("guard", opt.guard))
    seen = set()
    for key, name, t in model_index(upd):
        if name is None and id(t) not in seen:
            seen.add(id(t))
            segs.append(("model." + key, t))
    return segs


def check_save_point(upd, what):
    """The host side must stand where an eager loop has it after update n."""
    if upd.world > 1:
        raise ValueError(f"{what}: the process group has {upd.world} ranks; saving and resuming several ranks is not supported")
    if upd.sg is not None:
        if upd.prefetch_host:
            raise RuntimeError(f"{what} with prefetch_host=True: the helper thread has already pulled the next batch and drawn the next "
                               "update's host random numbers; build the update with prefetch_host=False to save from a replayed run")
        if upd.sg.sched._pending:
            raise RuntimeError(f"{what}: the first replay after the capture is already staged (its batch is pulled, its host random "
                               "numbers are drawn); run at least one update() first")


def extra_state(upd):
    pulled = upd._pulled_base + (upd.feed.pulls if upd.feed is not None else 0)
    return {"format": FORMAT, "num_updates": int(upd.n), **host_state(upd.device), "batches_pulled": int(pulled),
            "captures": int(upd.captures), "skip_run": int(upd._skip_run),
            "skip_run_first": -1 if upd._skip_run_first is None else int(upd._skip_run_first)}


def _signed(v):
    v = _cell(v)
    return v - (1 << 64) if v >> 63 else v


def assemble(host_segs, index, opt_meta, extra, digests=None):
    """The checkpoint dictionary from CPU copies of the segments.  host_segs {segment name: CPU tensor}: "pflat", "m", "v" (flat
    fp32), "guard" (int32, optional), "model.<key>" for every tensor of the model outside the flat buffer; index [(model key, name of
    the flat parameter behind it or None, shape, segment name or None)]; digests {segment: int} as the device computed them (the
    caller has verified them) or None: computed here."""
    where = {name: (off, n) for name, off, n in opt_meta["layout"]}
    model = {}
    for key, pname, shape, seg in index:
        if pname is not None:
            off, n = where[pname]
            model[key] = host_segs["pflat"][off:off + n].view(shape)
        elif seg in host_segs:
            model[key] = host_segs[seg]
        else:
            raise ValueError(f"checkpoint: no segment for {key}")
    optimizer = dict(opt_meta)
    optimizer["m"], optimizer["v"] = host_segs["m"], host_segs["v"]
    if "guard" in host_segs:
        optimizer["guard"] = [int(c) for c in host_segs["guard"].tolist()]
    if digests is None:
        digests = {name: host_digest(t) for name, t in host_segs.items()}
    return {"model": model, "optimizer": optimizer, "extra_state": extra, "digest": {k: _signed(v) for k, v in digests.items()}}


def _index_of(upd):
    """model_index() without the live tensors; keys that share one tensor outside the flat buffer share the first key's segment."""
    first, out = {}, []
    for key, pname, t in model_index(upd):
        seg = None
        if pname is None:
            seg = "model." + first.setdefault(id(t), key)
        out.append((key, pname, tuple(t.shape), seg))
    return out


def state_dict(upd):
    """PretrainUpdate.state_dict(): waits for the update's stream; CPU data only; no device memory is allocated."""
    check_save_point(upd, "state_dict()")
    if upd.stream is not None:
        upd.stream.synchronize()
        torch.cuda.synchronize(upd.device)
    segs = device_segments(upd)
    host = {name: t.detach().cpu().contiguous().reshape(-1) if name in ("pflat", "m", "v", "guard") else t.detach().cpu().contiguous()
            for name, t in segs}
    digests = {name: host_digest(t) for name, t in host.items()}
    if upd.opt.mirror is not None:
        digests["wflat"] = host_digest(upd.opt.wflat.cpu())
    return assemble(host, _index_of(upd), optimizer_meta(upd.opt), extra_state(upd), digests)


def segments_of(sd):
    """{segment name: CPU tensor} rebuilt from a checkpoint dictionary: what its digests (all but "wflat") were taken over."""
    opt = sd["optimizer"]
    pflat = torch.zeros(int(opt["numel"]), dtype=torch.float32)
    for name, off, n in opt["layout"]:
        if name not in sd["model"]:
            raise ValueError(f"checkpoint: parameter {name} of the saved layout is missing from the saved model")
        if sd["model"][name].numel() != n:
            raise ValueError(f"checkpoint: parameter {name} has {sd['model'][name].numel()} elements, the saved layout has {n}")
        pflat[off:off + n] = sd["model"][name].reshape(-1).float()
    out = {"pflat": pflat, "m": opt["m"], "v": opt["v"]}
    if "guard" in opt:
        out["guard"] = torch.tensor([int(c) for c in opt["guard"]], dtype=torch.int32)
    for k in sd["digest"]:
        if k.startswith("model."):
            if k[6:] not in sd["model"]:
                raise ValueError(f"checkpoint: segment {k} has a digest and no tensor")
            out[k] = sd["model"][k[6:]]
    return out


def verify(sd):
    """Recompute the digest of every saved segment; ValueError naming the first segment that differs."""
    for key in ("model", "optimizer", "extra_state", "digest"):
        if key not in sd:
            raise ValueError(f"checkpoint: no {key!r} entry")
    segs = segments_of(sd)
    for name in ("pflat", "m", "v") + (("guard",) if "guard" in segs else ()):
        if name not in sd["digest"]:
            raise ValueError(f"checkpoint: no digest for segment {name}")
    for name, t in segs.items():
        got, want = host_digest(t), _cell(sd["digest"][name])
        if got != want:
            raise ValueError(f"checkpoint: segment {name} does not match its digest ({got:#018x}, saved {want:#018x})")
    return sd


def load_state_dict(upd, sd):
    """PretrainUpdate.load_state_dict(): see the class; everything a load must restore, in one place."""
    if upd.world > 1:
        raise ValueError(f"load_state_dict(): the process group has {upd.world} ranks; saving and resuming several ranks is not supported")
    if upd.sg is not None:
        raise RuntimeError("load_state_dict() with a captured graph: load before prepare_graph()")
    opt, ex = upd.opt, sd["extra_state"]
    dev = upd.device
    index = model_index(upd)
    for key, pname, t in index:
        if pname is None:
            if key not in sd["model"]:
                raise ValueError(f"checkpoint: {key} is missing from the saved model")
            if tuple(sd["model"][key].shape) != tuple(t.shape):
                raise ValueError(f"checkpoint: {key} has shape {tuple(t.shape)}, the saved model has {tuple(sd['model'][key].shape)}")
    on = torch.cuda.stream(upd.stream) if upd.stream is not None else _Null()
    if upd.stream is not None:
        upd.stream.wait_stream(torch.cuda.current_stream(dev))
    with on:
        load_optimizer_state_dict(opt, sd["optimizer"], params=sd["model"], lr_scheduled=upd.lr_fn is not None)
        with torch.no_grad():
            for key, pname, t in index:
                if pname is None:
                    t.copy_(sd["model"][key].to(device=t.device, dtype=t.dtype))
        rebuild_images(opt)
        if opt.mirror is not None:
            if "wflat" not in sd["digest"]:
                raise ValueError("checkpoint: no digest of the bf16 image (segment wflat): it was saved from an fp32 update")
            got = host_digest(opt.wflat.cpu())       # (synchronises: a load is not on the training path)
            if got != _cell(sd["digest"]["wflat"]):
                raise ValueError(f"checkpoint: the rebuilt bf16 image differs from the one the Adam kernel had written (segment wflat: "
                                 f"{got:#018x}, saved {_cell(sd['digest']['wflat']):#018x})")
    if upd.stream is not None:
        torch.cuda.current_stream(dev).wait_stream(upd.stream)
    upd.n = int(ex["num_updates"])
    upd.model.set_num_updates(upd.n)
    if upd.lr_fn is not None:
        opt.lr = upd.lr_fn(upd.n)
    set_host_state(ex, dev)
    upd.captures = int(ex["captures"])
    upd._pulled_base = int(ex["batches_pulled"]) - (upd.feed.pulls if upd.feed is not None else 0)
    upd._skip_run = int(ex["skip_run"])
    upd._skip_run_first = None if int(ex["skip_run_first"]) < 0 else int(ex["skip_run_first"])
    # (statistics are not state: a new update's recorder starts empty and its entries carry on from num_updates)


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


# ---------------------------------------------------------------------------------------------------------------------------------
# a snapshot that does not stop training
# ---------------------------------------------------------------------------------------------------------------------------------
class _Shadow:
    """Device shadow of the state's segments + the descriptor tables of the two launches + the pinned host image.  Allocated on the
    first snapshot; the segments of an update never change size, and should a later snapshot need more (a model that grew a buffer),
    a larger block is allocated and the old one is KEPT -- nothing is freed while the update lives (the rule of the library's stream
    scratch: work that is still enqueued may read it)."""

    def __init__(self, upd):
        self.kept = []
        self.cap = 0
        # a stream of another priority: this runtime gives each priority level its own hardware queues, and a side stream that shares
        # a hardware queue with the update's stream puts the 30 ms copy IN FRONT of the next update (measured: profiles/
        # checkpoint_timing.json)
        self.side = torch.cuda.Stream(device=upd.device, priority=-1)
        self.sig = None

    def plan(self, upd):
        segs = device_segments(upd)
        for name, t in segs:
            if not t.is_contiguous():
                raise ValueError(f"snapshot(): segment {name} is not contiguous")
        sig = tuple((name, t.data_ptr(), t.numel() * t.element_size()) for name, t in segs)
        wf = upd.opt.wflat if upd.opt.mirror is not None else None
        sig += (("wflat", wf.data_ptr() if wf is not None else 0, wf.numel() * wf.element_size() if wf is not None else 0),)
        if sig == self.sig:
            return
        dev = upd.device
        nbytes = [n for _, _, n in sig[:-1]]
        offs, tot = [], 0
        for n in nbytes:
            offs.append(tot)
            tot += (n + 255) // 256 * 256
        tot = max(tot, 256)
        if tot > self.cap:
            if self.cap:
                self.kept.append((self.dev, self.host, self.cells, self.cells_host))
            self.dev = torch.empty(tot, dtype=torch.uint8, device=dev)
            self.host = torch.empty(tot, dtype=torch.uint8).pin_memory()
            self.cap = tot
        n = len(nbytes)
        base = self.dev.data_ptr()
        self.names = [name for name, _, _ in sig[:-1]]
        self.offs, self.nbytes = offs, nbytes
        prefix = Fn.batch_load_plan(nbytes)
        t = torch.tensor([a for _, a, _ in sig[:-1]] + [base + o for o in offs] + nbytes + prefix, dtype=torch.int64).to(dev)
        self.copy_table = (t, t[:n], t[n:2 * n], t[2 * n:3 * n], t[3 * n:])
        self.copy_chunks = prefix[-1]
        # the digest runs over the shadow and, as one more segment, over the LIVE bf16 image: read on the update's stream behind the
        # newest update and in front of the next one, it is the image that belongs to the shadowed master
        dsegs = [base + o for o in offs] + ([sig[-1][1]] if wf is not None else [])
        dbytes = nbytes + ([sig[-1][2]] if wf is not None else [])
        dprefix = Fn.batch_load_plan(dbytes)
        k = len(dsegs)
        d = torch.tensor(dsegs + dbytes + dprefix, dtype=torch.int64).to(dev)
        self.digest_table = (d, d[:k], d[k:2 * k], d[2 * k:])
        self.digest_chunks, self.n_digest = dprefix[-1], k
        if self.kept or getattr(self, "cells", None) is not None:
            self.kept.append((self.cells, self.cells_host))
        self.cells = torch.zeros(k, dtype=torch.int64, device=dev)
        self.cells_host = torch.zeros(k, dtype=torch.int64).pin_memory()
        self.has_wflat = wf is not None
        self.sig = sig


class Snapshot:
    """Handle of PretrainUpdate.snapshot().  done() never waits; result() waits for the copy, checks every host segment against the
    device's digest and returns the dictionary state_dict() returns."""

    def __init__(self, upd, shadow, event, index, opt_meta, extra, shapes):
        self._upd, self._sh, self._ev = upd, shadow, event
        self._index, self._meta, self._extra, self._shapes = index, opt_meta, extra, shapes
        self._sd = None
        self._taken = False

    def done(self):
        return self._taken or self._ev.query()

    def result(self):
        if self._taken:
            if self._sd is None:
                raise RuntimeError("Snapshot.result(): this snapshot failed its digest check")
            return self._sd
        self._ev.synchronize()
        sh = self._sh
        try:
            cells = [_cell(c) for c in sh.cells_host.tolist()]
            host, digests = {}, {}
            for i, (name, off, n) in enumerate(zip(sh.names, sh.offs, sh.nbytes)):
                raw = sh.host[off:off + n]
                got = host_digest(raw)
                if got != cells[i]:
                    raise ValueError(f"snapshot: segment {name} arrived on the host with digest {got:#018x}, the device computed "
                                     f"{cells[i]:#018x}")
                dtype, shape = self._shapes[name]
                host[name] = raw.clone().view(dtype).view(shape)      # (out of the pinned image: the next snapshot reuses it)
                digests[name] = got
            if sh.has_wflat:
                digests["wflat"] = cells[-1]
            sd = assemble(host, self._index, self._meta, self._extra, digests)
            self._sd = sd
            return sd
        finally:
            self._taken = True
            if self._upd._snapshot is self:
                self._upd._snapshot = None
            self._upd = None


def snapshot(upd):
    """PretrainUpdate.snapshot(): two launches on the update's stream, one asynchronous copy on a side stream, a handle at once."""
    check_save_point(upd, "snapshot()")
    if upd.stream is None:
        raise RuntimeError("snapshot() needs an update on a GPU; state_dict() works everywhere")
    if upd._snapshot is not None:
        raise RuntimeError("snapshot(): the previous snapshot is still in flight -- take its result() first (one pinned image, one shadow)")
    if upd._shadow is None:
        upd._shadow = _Shadow(upd)
    sh = upd._shadow
    sh.plan(upd)
    # the host part, read at the call
    index, meta, extra = _index_of(upd), optimizer_meta(upd.opt), extra_state(upd)
    shapes = {name: (t.dtype, (t.numel(),) if name in ("pflat", "m", "v", "guard") else tuple(t.shape)) for name, t in device_segments(upd)}
    upd.stream.wait_stream(torch.cuda.current_stream(upd.device))
    with torch.cuda.stream(upd.stream):
        _, src, dst, nbytes, prefix = sh.copy_table
        Fn.batch_load(src, dst, nbytes, prefix, len(sh.names), sh.copy_chunks)
        _, seg, dbytes, dprefix = sh.digest_table
        Fn.state_digest(seg, dbytes, dprefix, sh.n_digest, sh.digest_chunks, sh.cells)
        ready = torch.cuda.Event()
        ready.record()
    sh.side.wait_event(ready)
    with torch.cuda.stream(sh.side):
        sh.host.copy_(sh.dev, non_blocking=True)
        sh.cells_host.copy_(sh.cells, non_blocking=True)
        arrived = torch.cuda.Event()
        arrived.record()
    h = Snapshot(upd, sh, arrived, index, meta, extra, shapes)
    upd._snapshot = h
    return h


# ---------------------------------------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------------------------------------
def write_checkpoint(sd, path):
    """torch.save to a temporary file in the target's directory, fsync, os.replace: a killed process leaves the old file or the new
    one, never a torn one."""
    path = os.fspath(path)
    tmp = os.path.join(os.path.dirname(os.path.abspath(path)), f".{os.path.basename(path)}.tmp{os.getpid()}")
    try:
        with open(tmp, "wb") as f:
            torch.save(sd, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    try:      # (the directory entry too, where the platform lets a directory be opened)
        fd = os.open(os.path.dirname(os.path.abspath(path)), os.O_RDONLY)
        try:
            os.fsync(fd)
        finally:
            os.close(fd)
    except OSError:
        pass


def save_checkpoint(upd, path):
    write_checkpoint(snapshot(upd).result() if upd.stream is not None else state_dict(upd), path)


def load_checkpoint(path):
    """The dictionary for PretrainUpdate.load_state_dict(), its digests recomputed and checked (ValueError naming the segment)."""
    return verify(torch.load(os.fspath(path), map_location="cpu", weights_only=True))
