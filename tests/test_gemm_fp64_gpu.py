"""csrc/gemm.hip (st5_gemm, st5_gemm_tn_group) through the C ABI against the fp64 restatement of tests/gemm_reference.py, at the
smallest shapes at which each kernel can go wrong: partial row / column tiles, K tails, every ring wrap, the slow epilogue (N % 8 != 0 or
a C-class operand off 16-byte alignment), row-split and batched C layouts, every epilogue combination, the dropout counter rule of the
header (element counter = z M N + row N + col) with an independently computed mask, split-K immediate and deferred, grouped launches.

The bar (gemm_reference.bar_terms / bar_ratio, the functions gemm_reference.judge is made of, evaluated on the device), per ELEMENT of C, Cpre and asum, nothing in it from a kernel's output:
    |kernel - fp64| <= BAR max(|emulation - fp64|, ulp_out(fp64) / 2) + summation_floor(S, chain) (+ the GELU polynomials' documented bounds)
BAR = norm_reference.BAR = 4; S = |alpha| sum |a| |b| + |bias| carried through the activation's Lipschitz factor and 1 / (1 - p), plus |R| +
|beta C_old| (asum: sum |a| + |old|); chain = K + 16 epilogue operations (asum: K + 1, + the split count).  The reported ratio is
(|kernel - fp64| - floor) / max(|emulation - fp64|, ulp / 2), worst element.  Where one C is written by two launches in a row (deferred
split-K queued twice, two grouped problems on one output) the first launch's own bar is added to the second's: its error is carried.
Dropout cases are judged by value like every other: a dropped element must be R + beta C_old, a kept one the scaled value, and
tests/test_gemm_reference_cpu.py shows that a wrong mask bit lies far outside the tolerance for all but <= 1 % of the elements.

Every output -- C, Cpre and the asum column alike -- is NaN-filled (or holds the old contents that beta / asum accumulate onto) inside
a NaN buffer with GUARD elements behind it; the gaps of row-split / batched layouts, the columns between N and ld and the guard must come back bit-identical.  Operand tails
that must not be read (K tail, columns beyond the matrix) hold NaN.  Everything runs under util.poisoned_allocations(); one pass per test.
The measured ratios of an MI355X run are in profiles/gemm_fp64_ratios.txt."""
import math

import numpy as np
import pytest
import torch

from speecht5_amd import hip
from tests import gemm_reference as G
from tests.util import poisoned_allocations

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
DTYPES, IDS = [BF, FP], ["bf16", "fp32"]
DEFERRABLE = 16
_DEFAULTS = dict(nt_tile=0, deep_ring=(256, 4), nt_slots=5, glds=1, splitk_target=384, tn_phased=0, tn_group_tile=0)
# tile kernel -> st5_gemm_set_nt_tile, st5_gemm_set_deep_ring, st5_gemm_set_nt_slots (tests/test_gemm_nn_gpu.py): at these sizes every grid is
# "at most 256 blocks", so the 128 x 128 kernel runs the ring depth given here from 4 k-tiles on and its five-slot / two-stage form below.
TILES = {"128-ring4": (1, (256, 4), 5), "128-ring3": (1, (256, 3), 5), "128-slots5": (1, (0, 2), 5), "128-ring2": (1, (0, 2), 4),
         "m64": (5, (256, 4), 5), "first256": (2, (256, 4), 5), "phased": (3, (256, 4), 5), "phased-nostagger": (4, (256, 4), 5)}


class knobs:
    """The library's launch choices forced for the block; its defaults afterwards."""

    def __init__(self, **kw):
        self.v = dict(_DEFAULTS, **kw)

    @staticmethod
    def _set(v):
        L = hip.lib()
        for name, val in v.items():
            hip.check(getattr(L, "st5_gemm_set_" + name)(*(val if isinstance(val, tuple) else (val,))), "st5_gemm_set_" + name)

    def __enter__(self):
        self._set(self.v)

    def __exit__(self, *exc):
        self._set(_DEFAULTS)


def tile_knobs(tile):
    mode, deep, slots = TILES[tile]
    return knobs(nt_tile=mode, deep_ring=deep, nt_slots=slots)


# ---- running a problem of gemm_reference on the device ---------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Device:
    """The flat buffers of gemm_reference problems on the GPU: inputs uploaded once (by identity of the CPU tensor), outputs cloned from
    their uploaded initial state for every launch."""

    def __init__(self, dev):
        self.dev, self.cache, self.keep = dev, {}, []

    def buf(self, t):
        if id(t) not in self.cache:
            self.cache[id(t)] = t.to(self.dev)
            self.keep.append(t)
        return self.cache[id(t)]

    def operand(self, op, t=None):
        return hip.operand(self.buf(op.buf) if t is None else t, op.ld, op.off, op.rpb, op.bstride, op.seg, op.seg_stride, op.zs0, op.zs1)

    def args(self, p, outs=None):
        """(A, B, C operands, keyword arguments of hip.gemm, outs): outs = the fresh output buffers {C, Cpre, asum} of this launch."""
        outs = {} if outs is None else outs
        if "C" not in outs:
            outs["C"] = self.buf(p.C.buf).clone()
        if p.Cpre is not None:
            outs["Cpre"] = self.buf(p.Cpre.buf).clone()
        if p.asum is not None and "asum" not in outs:
            outs["asum"] = self.buf(p.asum).clone()
        kw = dict(bias_zs=p.bias_zs, batch=p.batch, zdiv=p.zdiv, act=p.act, flags=p.flags, alpha=p.alpha, beta=p.beta, dropout_p=p.dropout_p)
        if p.bias is not None:
            kw["bias"] = self.buf(p.bias)
        for nm in ("R", "P"):
            if getattr(p, nm) is not None:
                kw[nm] = self.operand(getattr(p, nm))
        if p.Cpre is not None:
            kw["Cpre"] = self.operand(p.Cpre, outs["Cpre"])
        if p.asum is not None:
            kw["asum"] = outs["asum"]
        seed = int(p.seed)
        if seed >> 63:      # a seed slot: the value lives in device memory, the argument is its address with bit 63 set
            slot = torch.tensor([G.resolve_seed(p)], dtype=torch.int64, device=self.dev)
            self.keep.append(slot)
            seed = (1 << 63) | slot.data_ptr()
        kw["seed"] = seed
        return self.operand(p.A), self.operand(p.B), self.operand(p.C, outs["C"]), kw, outs

    def run(self, p, dtype, outs=None, flags=0):
        a, b, c, kw, outs = self.args(p, outs)
        kw["flags"] |= flags
        hip.gemm(a, b, c, p.M, p.N, p.K, hip.dt(dtype), **kw)
        return outs

    def run_group(self, ps, dtype, outs_list, gates=None):
        lst = []
        for j, (p, outs) in enumerate(zip(ps, outs_list)):
            a, b, c, kw, _ = self.args(p, outs)
            lst.append((a, b, c, p.M, p.N, p.K, p.flags, p.beta, kw.get("asum"), gates[j].data_ptr() if gates and gates[j] is not None else 0))
        hip.gemm_tn_group(lst, hip.dt(dtype))


class Expect:
    """What a problem's outputs must be, on the device: per output tensor the element offsets, fp64 reference, max(|emulation - fp64|,
    ulp / 2), the floor, and the initial bits of the whole buffer with the mask of elements no launch may touch."""

    def __init__(self, p, dtype, dev, nsplit=1, carry=None):
        self.p, self.dtype, self.dev = p, dtype, dev
        ref, emu = G.gemm(p, dtype), G.gemm(p, dtype, emulate=True)
        self.ref, self.t = ref, {}
        self._add("C", p.C.buf, G.c_offsets(p.C, p), ref.C, emu.C, ref.S, ref.chain, ref.c_dtype, ref.extra, carry)
        if p.Cpre is not None:
            self._add("Cpre", p.Cpre.buf, G.c_offsets(p.Cpre, p), ref.Cpre, emu.Cpre, ref.S_pre, ref.chain, dtype, None, None)
        if p.asum is not None:
            self._add("asum", p.asum, np.arange(p.M), ref.asum, emu.asum, ref.S_asum, p.K + 1 + nsplit, FP, None, None)

    def _add(self, nm, before, offs, ref, emu, S, chain, out_dtype, extra, carry):
        d = lambda x: x.reshape(-1).to(self.dev)
        den, floor = G.bar_terms(ref, emu, S, chain, out_dtype, extra)
        if carry is not None:       # the error of the launch that produced C_old rides on this one's result
            den, floor = den + carry[0].reshape(den.shape), floor + carry[1].reshape(floor.shape)
        idx = torch.from_numpy(np.asarray(offs)).reshape(-1)
        free = torch.ones(before.numel(), dtype=torch.bool)
        free[idx] = False
        self.t[nm] = dict(idx=idx.to(self.dev), ref=d(ref), den=d(den), floor=d(floor), emu_err=(emu - ref).abs().max().item(),
                          free=free.to(self.dev), before=_bits(before.to(self.dev)), den_cpu=den, floor_cpu=floor)

    def carry(self):
        return self.t["C"]["den_cpu"], self.t["C"]["floor_cpu"]

    def measure(self, outs):
        """One row per output tensor, on the device: [kernel worst error, worst ratio, elements outside the output that changed]."""
        rows = []
        for nm, t in self.t.items():
            got = outs[nm].reshape(-1)
            vals = got[t["idx"]].double()
            err = (vals - t["ref"]).abs()
            ratio = G.bar_ratio(vals, t["ref"], t["den"], t["floor"]).max()
            touched = ((_bits(got) != t["before"]) & t["free"]).sum().double()
            rows.append(torch.stack([torch.nan_to_num(err, nan=math.inf).max(), ratio, touched]))
        return torch.stack(rows)

    def untouched(self, outs):
        """Number of bit patterns that differ from the initial state anywhere in the outputs (a gated launch must leave them all)."""
        return sum(int((_bits(outs[nm].reshape(-1)) != t["before"]).sum()) for nm, t in self.t.items())


class Ledger:
    """Measurements of one test, read back once at the end: prints one line per tensor and raises for every miss."""

    def __init__(self, family):
        self.family, self.rows = family, []

    def add(self, case, exp, outs):
        self.rows.append((case, exp, exp.measure(outs)))

    def settle(self):
        assert self.rows, "nothing was measured"
        table = iter(torch.cat([m for _, _, m in self.rows]).cpu().tolist())      # (one read-back for the whole test)
        missed = []
        for case, exp, _ in self.rows:
            for (nm, t), (ek, ratio, touched) in zip(exp.t.items(), table):
                print(f"gemm fp64 pin: {self.family} | {case} | {nm} | kernel {ek:.3e} emulation {t['emu_err']:.3e} ratio {ratio:.3f}")
                if not ratio <= G.BAR:
                    missed.append(f"{case} {nm}: kernel {ek:.3e}, emulation {t['emu_err']:.3e}, ratio {ratio:.3f} (bar {G.BAR})")
                if touched:
                    missed.append(f"{case} {nm}: {int(touched)} elements outside the output (gaps, tails, guard) were changed")
        assert not missed, f"{self.family}: {len(missed)} misses -- " + "; ".join(missed[:12])


def _name(dtype):
    return "bf16" if dtype == BF else "fp32"


# ---- (a) the general register-staged kernel ------------------------------------------------------------------------------------------
GEN_MS, GEN_NS, GEN_KS = G.GEN_MS, G.GEN_NS, G.GEN_KS
FORMS = {"NT": (False, False), "NN": (False, True), "TN": (True, True), "TT": (True, False)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", G.KINDS)
def test_general_kernel(cuda, dtype, kind):
    """st5_gemm_set_glds(0): every M x N x K of the lists in all four A / B storage forms (the values are the same, so one reference
    serves the four); N = 83 and 100 take the slow epilogue."""
    led = Ledger(f"general {_name(dtype)} {kind}")
    with poisoned_allocations(), knobs(glds=0):
        for M in GEN_MS:
            for N in GEN_NS:
                for K in GEN_KS:
                    v = G.inputs(M, N, K, bias_offset=3.0 if kind == "drop_res" else 0.0)
                    exp, dev = None, Device(cuda)
                    for form, (aks, bks) in FORMS.items():
                        p = G.case(M, N, K, dtype, kind, aks=aks, bks=bks, v=v)
                        exp = exp or Expect(p, dtype, cuda)
                        led.add(f"{M}x{N}x{K} {form}", exp, dev.run(p, dtype))
    led.settle()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", G.KINDS)
def test_general_kernel_unaligned_c(cuda, dtype, kind):
    """Fast-layout widths with C-class operands one element off 16-byte alignment: the slow epilogue at aligned dropout counters."""
    led = Ledger(f"general unaligned {_name(dtype)} {kind}")
    with poisoned_allocations(), knobs(glds=0):
        for M, N, K in G.UNALIGNED_SHAPES:
            p = G.case(M, N, K, dtype, kind, layout="unaligned")
            exp = Expect(p, dtype, cuda)
            assert not exp.ref.fast
            led.add(f"{M}x{N}x{K}", exp, Device(cuda).run(p, dtype))
    led.settle()


# ---- (b) every tile kernel, NT and B k-major --------------------------------------------------------------------------------------
TILE_MS, TILE_NS, TILE_KS = G.TILE_MS, G.TILE_NS, G.TILE_KS


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("tile", list(TILES))
def test_tile_kernels_bf16(cuda, tile, kind):
    """2, 3, 5 and 7 k-tiles (every ring wraps, the phased kernel sees an odd count); B as the NT operand, as a whole k-major matrix and
    as a column slice of a wider one (ld = N + 24).  (The first 256 x 256 kernel has no k-major form: those calls run on 128 x 128.)"""
    led = Ledger(f"tile {tile} bf16 {kind}")
    with poisoned_allocations(), tile_knobs(tile):
        for M in TILE_MS:
            for N in TILE_NS:
                for K in TILE_KS:
                    v = G.inputs(M, N, K, bias_offset=3.0 if kind == "drop_res" else 0.0)
                    exp, dev = None, Device(cuda)
                    for form, bks, pad in (("NT", False, 8), ("NN", True, 0), ("NN slice", True, 24)):
                        p = G.case(M, N, K, BF, kind, bks=bks, b_pad=pad, v=v)
                        exp = exp or Expect(p, BF, cuda)
                        led.add(f"{M}x{N}x{K} {form}", exp, dev.run(p, BF))
    led.settle()


@pytest.mark.parametrize("kind", G.KINDS)
def test_first_256_kernel_fp32(cuda, kind):
    led = Ledger(f"tile first256 fp32 {kind}")
    with poisoned_allocations(), tile_knobs("first256"):
        for M, N, K in G.FIRST256_FP32_SHAPES:     # 2, 3, 5, 7 k-tiles of 32
            p = G.case(M, N, K, FP, kind)
            led.add(f"{M}x{N}x{K}", Expect(p, FP, cuda), Device(cuda).run(p, FP))
    led.settle()


# ---- (c) the run-time-only epilogue combinations, one shape per kernel -----------------------------------------------------------
@pytest.mark.parametrize("kind", G.RT_KINDS)
def test_run_time_epilogues(cuda, kind):
    """ReLU, tanh and both LeakyReLUs forward and as DACT, GELU + dropout + R + Cpre + beta together, OUT_F32 with an fp32 R: the general
    kernel in both types (fast and slow layout) and every tile kernel."""
    led = Ledger(f"run-time {kind}")
    with poisoned_allocations():
        for dtype in DTYPES:
            for M, N, K in G.RT_GENERAL_SHAPES:
                p = G.case(M, N, K, dtype, kind)
                with knobs(glds=0):
                    led.add(f"general {_name(dtype)} {M}x{N}x{K}", Expect(p, dtype, cuda), Device(cuda).run(p, dtype))
        M, N, K = G.RT_TILE_SHAPE[BF]
        p = G.case(M, N, K, BF, kind)
        exp, dev = Expect(p, BF, cuda), Device(cuda)
        for tile in TILES:
            with tile_knobs(tile):
                led.add(f"{tile} bf16 {M}x{N}x{K}", exp, dev.run(p, BF))
        M, N, K = G.RT_TILE_SHAPE[FP]
        p = G.case(M, N, K, FP, kind)
        with tile_knobs("first256"):
            led.add(f"first256 fp32 {M}x{N}x{K}", Expect(p, FP, cuda), Device(cuda).run(p, FP))
    led.settle()


# ---- (d) dropout addressing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dropout_counter_rule(cuda, dtype):
    """Element counter = z M N + row N + col for every N and layout, the mask from attention_reference.keep_mask_flat: batch = 3 through
    zs1 and zs0 (the z M N term), row-split C and R, seed direct and through a slot, p = 0.1 and 0.5, on the general kernel and on what the
    default dispatch picks (K = 128: an LDS-DMA tile kernel in bf16 and fp32).
    N = 83 and 100 decide the rule for the slow layout: there a row's first counter is no multiple of 8 (N = 83: every other row starts at an
    odd counter, so the pair parity matters; N = 100: 8-vectors straddle the 64-element blocks, so the block key matters), and the
    epilogue has to evaluate such an 8-vector element by element (common.h dropout_scale), not with the aligned 8-wide form.  N = 136 with
    unaligned operands is the same layout at aligned counters."""
    led = Ledger(f"dropout {_name(dtype)}")
    with poisoned_allocations():
        for name, p in G.drop_cases(dtype):
            exp, dev = Expect(p, dtype, cuda), Device(cuda)
            with knobs(glds=0):
                led.add(f"{name} general", exp, dev.run(p, dtype))
            led.add(f"{name} default", exp, dev.run(p, dtype))
    led.settle()


# ---- (e) weight-gradient forms ---------------------------------------------------------------------------------------------------
def _host_splits(M, N, K, dtype, target=384):
    """st5_gemm's split-K rule restated (fp32 output, plain, N % 8 == 0): the number of slabs."""
    tiles, bk = ((M + 127) // 128) * ((N + 127) // 128), 64 if dtype == BF else 32
    nk = (K + bk - 1) // bk
    if not (tiles < 200 and nk >= 16):
        return 1
    ns = max(min((target + tiles - 1) // tiles, nk // 8), 1)
    per = (nk + ns - 1) // ns
    return (nk + per - 1) // per


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("asum", [False, True], ids=["", "asum"])
@pytest.mark.parametrize("beta", [0.0, 1.0], ids=["beta0", "beta1"])
def test_weight_gradient_form(cuda, dtype, beta, asum):
    """C[M, N] (+)= A^T B, both operands k-strided, fp32 C: without split-K, split in two by the host rule (which splits from 16 k-tiles on; 1088 is
    17 k-tiles of 64, 1160 adds a K tail), at three slabs of uneven length (K = 2176 with a target of 6 blocks), immediate and deferred reduction.  fp32
    runs the general kernel (its k-tile is 32: the same K are 34 and more tiles)."""
    led = Ledger(f"wgrad {_name(dtype)} beta={beta:g}{' asum' if asum else ''}")
    L = hip.lib()
    with poisoned_allocations():
        for M, N, K, target in ((136, 72, 256, 384), (264, 776, 130, 384), (136, 72, 1088, 384), (136, 72, 1160, 384), (136, 72, 2176, 6)):
            ns = _host_splits(M, N, K, dtype, target)
            if dtype == BF:
                assert ns == {256: 1, 130: 1, 1088: 2, 1160: 2, 2176: 3}[K]
            p = G.wgrad_case(M, N, K, dtype, beta, asum)
            exp, dev = Expect(p, dtype, cuda, nsplit=ns), Device(cuda)
            with knobs(splitk_target=target):
                led.add(f"{M}x{N}x{K} splits={ns}", exp, dev.run(p, dtype))
                if ns > 1:
                    hip.check(L.st5_gemm_defer_splitk(1, hip.stream()), "st5_gemm_defer_splitk")
                    try:
                        outs = dev.run(p, dtype, flags=DEFERRABLE)
                        hip.check(L.st5_gemm_flush_splitk(hip.stream()), "st5_gemm_flush_splitk")
                    finally:
                        hip.check(L.st5_gemm_defer_splitk(0, hip.stream()), "st5_gemm_defer_splitk")
                    led.add(f"{M}x{N}x{K} splits={ns} deferred", exp, outs)
    led.settle()


def test_deferred_split_k_same_output_twice(cuda):
    """The same C queued twice (tied weights) forces the early fold: C = C0 + X1, then + X2."""
    led = Ledger("wgrad bf16 deferred twice")
    L = hip.lib()
    with poisoned_allocations():
        p1 = G.wgrad_case(136, 72, 1088, BF, 1.0, True)
        e1 = Expect(p1, BF, cuda, nsplit=2)
        p2 = G.wgrad_case(136, 72, 1088, BF, 1.0, True, seed=1)
        p2.C.buf[torch.from_numpy(G.c_offsets(p2.C, p2)).reshape(-1)] = e1.ref.C.reshape(-1).float()      # C_old of the second = the first's fp64 result
        p2.asum = G.asum_buf(e1.ref.asum)
        e2 = Expect(p2, BF, cuda, nsplit=2, carry=e1.carry())
        e2.t["C"]["before"], e2.t["asum"]["before"] = e1.t["C"]["before"], e1.t["asum"]["before"]
        dev = Device(cuda)
        hip.check(L.st5_gemm_defer_splitk(1, hip.stream()), "st5_gemm_defer_splitk")
        try:
            outs = dev.run(p1, BF, flags=DEFERRABLE)
            dev.run(p2, BF, outs=outs, flags=DEFERRABLE)
            hip.check(L.st5_gemm_flush_splitk(hip.stream()), "st5_gemm_flush_splitk")
        finally:
            hip.check(L.st5_gemm_defer_splitk(0, hip.stream()), "st5_gemm_defer_splitk")
        # asum: the second launch's old contents were the first's result, whose own bar rides along
        t1, t2 = e1.t["asum"], e2.t["asum"]
        t2["den"], t2["floor"] = t2["den"] + t1["den"], t2["floor"] + t1["floor"]
        led.add("136x72x1088 twice", e2, outs)
    led.settle()


@pytest.mark.parametrize("mode", [1, 2], ids=["stagger", "nostagger"])
def test_weight_gradient_phased(cuda, mode):
    led = Ledger(f"wgrad bf16 phased mode {mode}")
    with poisoned_allocations(), knobs(tn_phased=mode):
        for M, N, K in ((256, 256, 512), (256, 512, 576)):
            for beta, asum in ((0.0, False), (1.0, True)):
                p = G.wgrad_case(M, N, K, BF, beta, asum)
                ns = max(min(256 // ((M // 256) * (N // 256)), ((K + 63) // 64) // 4), 1)
                led.add(f"{M}x{N}x{K} beta={beta:g}", Expect(p, BF, cuda, nsplit=ns), Device(cuda).run(p, BF))
    led.settle()


SMALL_GROUP = ((136, 72, 256), (264, 72, 320), (8, 8, 64))
PHASED_GROUP = ((256, 256, 512), (256, 512, 576), (512, 256, 512))          # tests/test_gemm_epilogue_loads_gpu.py


def _group(cuda, led, name, shapes, beta, gated=None):
    ps = [G.wgrad_case(M, N, K, BF, beta, True, seed=j) for j, (M, N, K) in enumerate(shapes)]
    exps, dev = [Expect(p, BF, cuda) for p in ps], Device(cuda)
    outs = [dict() for _ in ps]
    for p, o in zip(ps, outs):
        dev.args(p, o)
    gates = None
    if gated is not None:
        keep0 = torch.zeros(1, device=cuda)
        dev.keep.append(keep0)
        gates = [keep0 if j == gated else None for j in range(len(ps))]
    dev.run_group(ps, BF, outs, gates)
    for j, (e, o, s) in enumerate(zip(exps, outs, shapes)):
        if j != gated:
            led.add(f"{name} {s[0]}x{s[1]}x{s[2]} beta={beta:g}", e, o)
    return exps, outs


@pytest.mark.parametrize("beta", [0.0, 1.0], ids=["beta0", "beta1"])
def test_grouped_weight_gradients(cuda, beta):
    """st5_gemm_tn_group: three problems of the 128 x 128 class, three of the phased class, a mixed list (two launches), and one problem
    under a gate at 0 whose C and asum must stay bit-identical."""
    assert all(hip.lib().st5_gemm_tn_group_is_phased(*s) for s in PHASED_GROUP) and not any(hip.lib().st5_gemm_tn_group_is_phased(*s) for s in SMALL_GROUP)
    led = Ledger(f"group bf16 beta={beta:g}")
    with poisoned_allocations():
        _group(cuda, led, "small", SMALL_GROUP, beta)
        _group(cuda, led, "phased", PHASED_GROUP, beta)
        _group(cuda, led, "mixed", (SMALL_GROUP[0], PHASED_GROUP[0], SMALL_GROUP[1], PHASED_GROUP[1]), beta)
        with knobs(tn_group_tile=1):
            _group(cuda, led, "phased shapes on 128x128", PHASED_GROUP[:2], beta)
        for shapes in (SMALL_GROUP, PHASED_GROUP):
            exps, outs = _group(cuda, led, "gated", shapes, beta, gated=1)
            torch.cuda.synchronize()
            assert exps[1].untouched(outs[1]) == 0, "a problem under a gate at 0 changed its C or asum"
    led.settle()


def test_grouped_weight_gradients_on_one_output(cuda):
    """Two problems of one list writing the same C and asum run one after the other: C0 + X1 + X2."""
    led = Ledger("group bf16 same output")
    with poisoned_allocations():
        for M, N, K in ((136, 72, 256), (256, 256, 512)):
            p1 = G.wgrad_case(M, N, K, BF, 1.0, True)
            e1 = Expect(p1, BF, cuda)
            p2 = G.wgrad_case(M, N, K, BF, 1.0, True, seed=1)
            p2.C.buf[torch.from_numpy(G.c_offsets(p2.C, p2)).reshape(-1)] = e1.ref.C.reshape(-1).float()
            p2.asum = G.asum_buf(e1.ref.asum)
            e2 = Expect(p2, BF, cuda, carry=e1.carry())
            t1, t2 = e1.t["asum"], e2.t["asum"]
            t2["den"], t2["floor"] = t2["den"] + t1["den"], t2["floor"] + t1["floor"]
            e2.t["C"]["before"], t2["before"] = e1.t["C"]["before"], t1["before"]
            dev, outs = Device(cuda), {}
            dev.args(p1, outs)
            dev.run_group([p1, p2], BF, [outs, outs])
            led.add(f"{M}x{N}x{K} twice", e2, outs)
    led.settle()


# ---- (f) addressing --------------------------------------------------------------------------------------------------------------
def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_addressing_batched_heads(cuda, dtype):
    """q k^T and P V per (batch, head) straight out of a fused [B T, 3 d] projection buffer (zs0 / zs1 / zdiv, off), scores into
    [B H, T, lds] with NaN between T and lds, the context back into [B T, d]."""
    g = torch.Generator().manual_seed(5)
    Bn, H, T, hd = 2, 3, 70, 64
    d, lds = H * hd, 72
    qkv = torch.full((Bn * T * 3 * d + G.GUARD,), G.NAN, dtype=dtype)
    qkv[:Bn * T * 3 * d] = _rand(g, Bn * T * 3 * d).to(dtype)
    q, k, vv = (G.Op(qkv, 3 * d, off=i * d, zs0=T * 3 * d, zs1=hd) for i in range(3))
    S = G.make_op(dtype, T, T, None, Bn * H, H, ld=lds, zs0=H * T * lds, zs1=T * lds)
    p1 = G.problem(q, k, S, T, T, hd, batch=Bn * H, zdiv=H, alpha=0.125)
    Pv = G.make_op(dtype, T, T, torch.softmax(_rand(g, Bn * H, T, T), -1), Bn * H, H, ld=lds, zs0=H * T * lds, zs1=T * lds)
    O = G.make_op(dtype, T, hd, None, Bn * H, H, ld=d, zs0=T * d, zs1=hd)
    p2 = G.problem(Pv, vv, O, T, hd, T, batch=Bn * H, zdiv=H, flags=G.B_KSTRIDED)
    led = Ledger(f"addressing heads {_name(dtype)}")
    with poisoned_allocations():
        for name, p in (("qk", p1), ("pv", p2)):
            exp, dev = Expect(p, dtype, cuda), Device(cuda)
            with knobs(glds=0):
                led.add(f"{name} general", exp, dev.run(p, dtype))
            led.add(f"{name} default", exp, dev.run(p, dtype))
    led.settle()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_addressing_convolutions(cuda, dtype):
    """Strided Conv1d as implicit GEMM on channels-last rows (overlapping rows, A row-split per utterance) + GELU; grouped pos-conv through
    K segments (seg / seg_stride, one batch index per group, bias_zs)."""
    g = torch.Generator().manual_seed(11)
    led = Ledger(f"addressing conv {_name(dtype)}")
    cases = []
    Bn, L, Cin, Cout = 3, 101, 64, 72
    for k, stride in ((3, 2), (2, 2)):
        Lo = (L - k) // stride + 1
        x = torch.full((Bn * L * Cin + G.GUARD,), G.NAN, dtype=dtype)
        x[:Bn * L * Cin] = _rand(g, Bn * L * Cin).to(dtype)
        W = G.ab_op(_rand(g, Cout, k * Cin) / math.sqrt(k * Cin), dtype, False)
        Y = G.make_op(dtype, Bn * Lo, Cout, None, ld=G.ceil8(Cout) + 8)
        cases.append((f"conv k={k} stride={stride}", G.problem(G.Op(x, stride * Cin, rpb=Lo, bstride=L * Cin), W, Y, Bn * Lo, Cout, k * Cin, act=G.ACT_GELU)))
    Bn, T, C, Gr, k = 2, 50, 64, 4, 16
    cg, Tp = C // Gr, T + k
    xp = torch.full((Bn * Tp * C + G.GUARD,), G.NAN, dtype=dtype)
    xp[:Bn * Tp * C] = _rand(g, Bn * Tp * C).to(dtype)
    Wg = G.make_op(dtype, cg, k * cg, _rand(g, Gr, cg, k * cg) / math.sqrt(k * cg), Gr, ld=k * cg, zs0=cg * k * cg)
    Y = G.make_op(dtype, Bn * T, cg, None, Gr, ld=C, zs0=cg)         # (the groups interleave in Y's rows: no gaps, only the guard)
    cases.append(("pos-conv groups", G.problem(G.Op(xp, C, rpb=T, bstride=Tp * C, seg=cg, seg_stride=C, zs0=cg), Wg, Y, Bn * T, cg, k * cg, batch=Gr,
                                              bias=_rand(g, C), bias_zs=cg, act=G.ACT_GELU)))
    with poisoned_allocations():
        for name, p in cases:
            exp, dev = Expect(p, dtype, cuda), Device(cuda)
            with knobs(glds=0):
                led.add(f"{name} general", exp, dev.run(p, dtype))
            led.add(f"{name} default", exp, dev.run(p, dtype))
    led.settle()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rpb", G.ROWSPLIT_RPBS)
def test_addressing_row_split(cuda, dtype, rpb):
    """A, C and P split every rpb rows with halo rows behind each block (the convolution data gradients through the GELU): blocks end
    inside 64-row wave tiles, the last tile is partial; also bias + dropout + R into the same layout."""
    led = Ledger(f"addressing rowsplit {_name(dtype)} rpb={rpb}")
    with poisoned_allocations():
        for kind in ("dact", "drop_res", "gelu_pre", "beta"):
            p = G.rowsplit_case(dtype, kind, rpb)
            exp, dev = Expect(p, dtype, cuda), Device(cuda)
            with knobs(glds=0):
                led.add(f"{kind} general", exp, dev.run(p, dtype))
            if dtype == BF:
                for tile in TILES:
                    with tile_knobs(tile):
                        led.add(f"{kind} {tile}", exp, dev.run(p, BF))
            else:
                led.add(f"{kind} default", exp, dev.run(p, dtype))
    led.settle()
