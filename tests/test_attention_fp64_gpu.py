"""The fused attention kernels (csrc/flash_attn2.hip, through functional._flash_fwd / _flash_bwd as training calls them) against
the fp64 reference of tests/attention_reference.py at recipe shapes, dropout included.

Bars: O and dQ per (b, h, query row), dK and dV per (b, h, key row), dPE per bucket row; metric ||kernel - fp64|| / max(||fp64 row||,
2^-8 * largest row norm of the tensor).  Each tensor's worst row is held to 4x the worst row of the bf16 emulation (the same
arithmetic in fp32 with the kernels' bf16 rounding points), the LSE to 4x the emulation's absolute error + 1e-6; the emulation's
own worst row is asserted to be non-zero and <= 2^-6.  For dQ, dK and dPE the floor of a row also covers
128x the bound on what rounding O to bf16 before D = dO . O does to it (row_metric).  The dropout masks come from the numpy restatement of the counter RNG, bit for bit
(test_fused_dropout_masks_bit_exact reads them back exactly from every place a fused kernel applies one)."""

import numpy as np
import pytest
import torch

from speecht5_amd import functional as Fn
from speecht5_amd import hip
from tests import attention_reference as R
from tests.util import poisoned_allocations

pytestmark = pytest.mark.gpu

HD = 64
MAXREL = 160
BAR = 4.0
SEED = 0x5EED_0000_1234


def _bf(x):
    return x.to(torch.bfloat16)


def _heads(x, B, T, H, col=0):
    """[B*T, ld] columns col .. col + H*HD -> [B, H, T, HD] (fp64, CPU)."""
    return x[:, col:col + H * HD].double().cpu().view(B, T, H, HD).permute(0, 2, 1, 3)


def _kpm(B, S, lens):
    if lens is None or all(n == S for n in lens):
        return None
    m = torch.zeros(B, S, dtype=torch.uint8)
    for b, n in enumerate(lens):
        m[b, n:] = 1
    return m


def case_inputs(B, H, T, S, rel, lens, p, kv_cols=None):
    """bf16 inputs (CPU) of one attention call in the model's packed layouts: x [B*T, 3d] (self attention, T == S) or
    xq [B*T, d] and xkv [B*S, ld] with this layer's keys / values at columns off .. off + 2d; dout [B*T, d]; pe; kpm."""
    g = torch.Generator().manual_seed(B * 1000003 + H * 10007 + T * 101 + S + int(p * 10))
    d = H * HD
    c = dict(self_attn=T == S and kv_cols is None, d=d)
    c["pe"] = _bf(torch.randn(2 * MAXREL, HD, generator=g) * 0.5) if rel else None
    c["kpm"] = _kpm(B, S, lens)
    c["dout"] = _bf(torch.randn(B * T, d, generator=g))
    if c["self_attn"]:
        c["x"] = _bf(torch.randn(B * T, 3 * d, generator=g))
        c["q"], c["k"], c["v"] = _heads(c["x"], B, T, H, 0), _heads(c["x"], B, T, H, d), _heads(c["x"], B, T, H, 2 * d)
    else:
        ld, off = kv_cols if kv_cols is not None else (2 * d, 0)
        c["ld"], c["off"] = ld, off
        c["xq"] = _bf(torch.randn(B * T, d, generator=g))
        c["xkv"] = _bf(torch.randn(B * S, ld, generator=g))
        c["q"], c["k"], c["v"] = _heads(c["xq"], B, T, H), _heads(c["xkv"], B, S, H, off), _heads(c["xkv"], B, S, H, off + d)
    return c


def references(c, B, H, T, S, rel, causal, p, seed=SEED):
    """fp64 reference and bf16 emulation of one case (CPU)."""
    keep = (lambda bh: R.keep_mask_attention(seed, p, B * H, T, S, rows=[bh])[0]) if p > 0 else None
    args = (c["q"], c["k"], c["v"], _heads(c["dout"], B, T, H), c["pe"].double() if rel else None, MAXREL if rel else 0, c["kpm"],
            causal, keep, p)
    return R.attention_fwd_bwd_fp64(*args), R.attention_bf16_emulation(*args)


def run_fused(B, H, T, S, rel, causal, lens, p, seed=SEED, kv_cols=None):
    """Inputs, kernel outputs and both references of one attention call.  kv_cols = (ld, off): cross attention whose keys /
    values are columns off .. off + 2d of an all-layer projection (KVShare), dK / dV written into a sentinel-filled buffer."""
    c = case_inputs(B, H, T, S, rel, lens, p, kv_cols)
    d = c["d"]
    dev = torch.device("cuda:0")
    self_attn, pe, kpm, dout = c["self_attn"], c["pe"], c["kpm"], c["dout"]
    if self_attn:
        X = c["x"].to(dev)
        qa, ka, va = (X, 3 * d, 0), (X, 3 * d, d), (X, 3 * d, 2 * d)
        G = torch.full((B * T, 3 * d), float("nan"), dtype=torch.bfloat16, device=dev)
        ga, gk, gv = (G, 3 * d, 0), (G, 3 * d, d), (G, 3 * d, 2 * d)
    else:
        ld, off = c["ld"], c["off"]
        XQ, XKV = c["xq"].to(dev), c["xkv"].to(dev)
        qa, ka, va = (XQ, d, 0), (XKV, ld, off), (XKV, ld, off + d)
        GQ = torch.full((B * T, d), float("nan"), dtype=torch.bfloat16, device=dev)
        GKV = torch.full((B * S, ld), float("nan") if kv_cols is None else -7.25, dtype=torch.bfloat16, device=dev)
        ga, gk, gv = (GQ, d, 0), (GKV, ld, off), (GKV, ld, off + d)
    PE = pe.to(dev) if rel else None
    KP = kpm.to(dev) if kpm is not None else None
    with poisoned_allocations():
        ctx, lse, qp = Fn._flash_fwd(qa, ka, va, B, H, T, S, HD, PE, MAXREL if rel else 0, KP, causal, p, seed, save_qp=rel)
        dpe = Fn._flash_bwd(dout.to(dev), ctx, lse, qa, ka, va, ga, gk, gv, B, H, T, S, HD, PE, rel, MAXREL if rel else 0, KP, causal,
                            p, seed, qp=qp, pe_t=PE.t().contiguous() if rel else None)
    torch.cuda.synchronize()
    if self_attn:
        kern = dict(dq=_heads(G, B, T, H, 0), dk=_heads(G, B, T, H, d), dv=_heads(G, B, T, H, 2 * d))
    else:
        kern = dict(dq=_heads(GQ, B, T, H), dk=_heads(GKV, B, S, H, gk[2]), dv=_heads(GKV, B, S, H, gv[2]))
        if kv_cols is not None:   # every column outside this layer's [K | V] keeps the sentinel, bit for bit
            keepcols = torch.ones(kv_cols[0], dtype=torch.bool)
            keepcols[kv_cols[1]:kv_cols[1] + 2 * d] = False
            sent = GKV[:, keepcols.to(dev)].cpu()
            assert torch.equal(sent.view(torch.int16), torch.full_like(sent, -7.25).view(torch.int16)), "KV-share: foreign columns written"
    kern.update(o=_heads(ctx, B, T, H), lse=lse.double().cpu().view(B, H, T), dpe=dpe.double().cpu() if rel else None)
    ref, emu = references(c, B, H, T, S, rel, causal, p, seed)
    return kern, ref, emu, kpm


def row_metric(got, ref, rho=None):
    """worst row of ||got - ref|| / max(||ref row||, 2^-8 * largest row norm, 2^7 * rho row), rows = all leading dims.  rho (dQ, dK,
    dPE): the most that rounding O to bf16 before D = dO . O can move the row (attention_reference: every fused kernel and the
    emulation take D from the bf16 O).  Where dS cancels -- it vanishes exactly for a query with one visible key, e.g. the first
    causal query or a one-key batch item -- that rounding is all that is left, and the row is judged against 128x its bound."""
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    rn = ref.norm(dim=1)
    den = torch.clamp(rn, min=2.0 ** -8 * rn.max().item())
    if rho is not None:
        den = torch.maximum(den, 2.0 ** 7 * rho.double().reshape(-1))
    err = (got - ref).norm(dim=1)
    # (a row that is exactly 0 with nothing to bound it -- no visible key, no (query, key) pair in the bucket -- must be exactly 0)
    return torch.where(err == 0, torch.zeros_like(err), err / den.clamp(min=1e-300)).max().item()


def check_case(name, kern, ref, emu, kpm, B, H, T, S, tail=False):
    for nm in ("o", "dq", "dk", "dv", "dpe"):
        if ref[nm] is None:
            continue
        assert torch.isfinite(kern[nm]).all(), f"{name} {nm}: non-finite values"
        rho = ref["rho"].get(nm)
        e_k, e_e = row_metric(kern[nm], ref[nm], rho), row_metric(emu[nm], ref[nm], rho)
        assert e_e <= 2.0 ** -6, f"{name} {nm}: emulation error {e_e:.3e} (the bar would be meaningless)"
        if e_e == 0 and tail:   # one visible key and no dropout: O = v exactly, in the emulation and the kernel alike
            assert e_k <= 1e-6, f"{name} {nm}: {e_k:.3e} where the emulation is exact"
            continue
        assert e_e > 0, f"{name} {nm}: the emulation equals fp64 (the bar would be vacuous)"
        print(f"attention fp64 pin: {name}: {nm} worst row kernel {e_k:.3e} emulation {e_e:.3e} ratio {e_k / e_e:.3f}")
        assert e_k <= BAR * e_e, f"{name} {nm}: worst row {e_k:.3e} > {BAR} x emulation {e_e:.3e}"
    if kpm is not None:   # padded keys: dK / dV rows exactly 0
        pad = kpm.bool()[:, None, :, None].expand(B, H, S, HD)
        assert torch.all(kern["dk"][pad] == 0) and torch.all(kern["dv"][pad] == 0), f"{name}: padded key rows not zero"
    lk, lr, le = kern["lse"], ref["lse"], emu["lse"]
    assert torch.equal(torch.isinf(lk), torch.isinf(lr)) and not torch.isnan(lk).any(), f"{name}: LSE +inf pattern"
    fin = torch.isfinite(lr)
    if fin.any():
        ea, ek = (le[fin] - lr[fin]).abs().max().item(), (lk[fin] - lr[fin]).abs().max().item()
        print(f"attention fp64 pin: {name}: lse worst row kernel {ek:.3e} emulation {ea:.3e} ratio {ek / max(ea, 1e-12):.3f}")
        assert ek <= BAR * ea + 1e-6, f"{name} lse: {ek:.3e} > {BAR} x {ea:.3e} + 1e-6"


# name, B, H, T, S, pe, causal, key lengths (None = full)
CASES = [
    ("base_encoder_10s", 2, 12, 499, 499, True, False, [499, 399]),
    ("large_heads_max_len", 4, 16, 780, 780, True, False, [780, 650, 401, 130]),
    ("odd_grid", 3, 12, 257, 257, True, False, [257, 200, 64]),
    ("text_decoder", 4, 12, 512, 512, False, True, [512, 512, 512, 400]),
    ("speech_decoder", 2, 12, 313, 313, False, True, None),
    ("asr_cross", 2, 12, 100, 499, False, False, [499, 399]),
    ("tts_cross_T_gt_S", 4, 12, 300, 100, False, False, [100, 87, 64, 1]),
    ("clipped_buckets", 1, 12, 700, 700, True, False, None),
    ("keys_past_unfused_limit", 1, 12, 200, 5000, False, False, None),
]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_attention_recipe_shapes(cuda, case, p):
    name, B, H, T, S, rel, causal, lens = case
    kern, ref, emu, kpm = run_fused(B, H, T, S, rel, causal, lens, p)
    check_case(f"{name} p={p}", kern, ref, emu, kpm, B, H, T, S)


TAILS = [(T, S) for T in (1, 65, 129) for S in (1, 7, 65, 129)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("T,S", TAILS)
def test_fused_attention_tails(cuda, T, S, pad, p):
    B, H = 2, 4
    same = T == S
    lens = [S, S - 1] if pad else None
    kern, ref, emu, kpm = run_fused(B, H, T, S, same, same, lens, p)
    check_case(f"tails T={T} S={S} pad={pad} p={p}", kern, ref, emu, kpm, B, H, T, S, tail=True)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_fused_attention_kv_share_columns(cuda, p):
    B, H, T, S = 2, 12, 100, 499
    d = H * HD
    kern, ref, emu, kpm = run_fused(B, H, T, S, False, False, [499, 399], p, kv_cols=(12 * d, 4 * d))
    check_case(f"kv share p={p}", kern, ref, emu, kpm, B, H, T, S)


def test_fused_attention_all_keys_padded_convention(cuda):
    B, H, T, S = 2, 4, 64, 64
    kern, ref, emu, kpm = run_fused(B, H, T, S, False, False, [64, 0], 0.0)
    assert torch.all(kern["o"][1] == 0) and torch.all(torch.isinf(kern["lse"][1]) & (kern["lse"][1] > 0))
    for nm in ("dq", "dk", "dv"):
        assert torch.all(kern[nm][1] == 0), nm
    check_case("all keys padded", kern, ref, emu, kpm, B, H, T, S)


# ---- dropout masks, bit for bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_fused_dropout_masks_bit_exact(cuda, p):
    """Reads back exactly every dropout mask the fused kernels apply.  T = 64, q_i = e_i, k_j = v_j = e_(j mod 64), item b sees only
    key tile b (S = 256: counter stride 256, tiles 0..3), so P[i][64b + c] = exp(scale [c == i]) / (63 + exp(scale)) is known:
      forward            O[i][c] = P M / keep                                     (fwd_kernel, P before P . V)
      dkv kernel, dV     dO_i = e_i:  dV[64b + c][i] = P M / keep                  (bwd_dkv_kernel, P before dO^T . P)
      dq kernel, dS      dO_i = 1:    dQ[i][c] = scale P (M / keep - D_i)          (bwd_dq_kernel, dP before dS)
      dkv kernel, dS     dO_i = 1:    dK[64b + c][i] = scale P (M / keep - D_i)    (bwd_dkv_kernel, dP before dS)
    with D_i = sum_c O[i][c] (the kernels take D from the bf16 O).  The probe holds draws equal to the threshold (where >= and >
    differ) in every kernel's region."""
    B, H, T, S = 4, 48, 64, 256
    d = H * HD
    dev = cuda
    seed = SEED + 17
    scale = HD ** -0.5
    ik = R.inv_keep(p)
    kpm = torch.ones(B, S, dtype=torch.uint8)
    for b in range(B):
        kpm[b, 64 * b:64 * b + 64] = 0
    eye = torch.eye(HD).repeat(S // HD, 1)                                      # [S, 64]: row j = e_(j mod 64)
    kvh = eye[None, :, None, :].expand(B, S, H, HD).reshape(B * S, d)
    kv = torch.cat([kvh, kvh], 1).to(torch.bfloat16).to(dev)
    q = torch.eye(T, HD)[None, :, None, :].expand(B, T, H, HD).reshape(B * T, d).to(torch.bfloat16).to(dev)
    P = np.where(np.eye(T, HD, dtype=bool), np.exp(scale), 1.0) / (63 + np.exp(scale))   # [i, c]
    draws = R.draws_attention(seed, B * H, T, S)
    thresh = R.dropout_thresh(p)
    vis = np.zeros((B, 1, 1, S), dtype=bool)
    for b in range(B):
        vis[b, ..., 64 * b:64 * b + 64] = True
    M = (draws.reshape(B, H, T, S) >= thresh)
    assert ((draws.reshape(B, H, T, S) == thresh) & vis).sum() >= 3, "probe holds no draw at the threshold"
    Mv = np.stack([M[b, :, :, 64 * b:64 * b + 64] for b in range(B)])        # [B, H, T(i), 64(c)]
    KP = kpm.to(dev)

    def tile_of_keys(g):   # [B*S, d] key rows -> [B, H, i (= d), c] of each item's own tile
        t = g.double().cpu().view(B, S, H, HD).permute(0, 2, 3, 1).numpy()
        return np.stack([t[b, :, :, 64 * b:64 * b + 64] for b in range(B)])

    with poisoned_allocations():
        ctx, lse, _ = Fn._flash_fwd((q, d, 0), (kv, 2 * d, 0), (kv, 2 * d, d), B, H, T, S, HD, None, 0, KP, False, p, seed)
    o = ctx.double().cpu().view(B, T, H, HD).permute(0, 2, 1, 3).numpy()
    assert np.array_equal(o != 0, Mv), f"forward mask: {((o != 0) ^ Mv).sum()} elements differ"
    dq = torch.full((B * T, d), float("nan"), dtype=torch.bfloat16, device=dev)
    dkv = torch.full((B * S, 2 * d), float("nan"), dtype=torch.bfloat16, device=dev)

    def backward(dout):
        with poisoned_allocations():
            Fn._flash_bwd(dout, ctx, lse, (q, d, 0), (kv, 2 * d, 0), (kv, 2 * d, d), (dq, d, 0), (dkv, 2 * d, 0), (dkv, 2 * d, d),
                          B, H, T, S, HD, None, False, 0, KP, False, p, seed)
        torch.cuda.synchronize()

    backward(torch.eye(T, HD)[None, :, None, :].expand(B, T, H, HD).reshape(B * T, d).to(torch.bfloat16).to(dev))
    dv = tile_of_keys(dkv[:, d:])
    assert np.array_equal(dv != 0, Mv), f"dkv mask on P (dV): {((dv != 0) ^ Mv).sum()} elements differ"
    backward(torch.ones(B * T, d, dtype=torch.bfloat16, device=dev))
    D = o.sum(-1, keepdims=True)                                                    # [B, H, T, 1]
    dqn = dq.double().cpu().view(B, T, H, HD).permute(0, 2, 1, 3).numpy()           # [B, H, i, c]
    dkn = tile_of_keys(dkv[:, :d])                                                  # [B, H, i, c]
    for what, g in (("dq kernel mask on dP (dQ)", dqn), ("dkv kernel mask on dP (dK)", dkn)):
        kept = g / (scale * P) + D > ik / 2                                         # kept: M / keep = ik, dropped: 0
        assert np.array_equal(kept, Mv), f"{what}: {(kept ^ Mv).sum()} elements differ"


def test_rng_restatement_equals_st5_dropout(cuda):
    """Flat counter layout (st5_dropout on ones), n not a multiple of 8, fp32 and bf16, bit for bit."""
    n, p, seed = 1_000_003, 0.1, 987654321
    keep = R.keep_mask_flat(seed, p, np.arange(n, dtype=np.uint64))
    for dt, code in ((torch.float32, hip.F32), (torch.bfloat16, hip.BF16)):
        ones = torch.ones(n, dtype=dt, device=cuda)
        out = torch.full((n,), float("nan"), dtype=dt, device=cuda)
        hip.check(hip.lib().st5_dropout(ones.data_ptr(), out.data_ptr(), n, p, seed, code, hip.stream()), "st5_dropout")
        want = torch.from_numpy(keep.astype(np.float32) * np.float32(R.inv_keep(p))).to(dt)
        assert torch.equal(out.cpu().view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                           want.view(torch.int16 if dt == torch.bfloat16 else torch.int32)), dt


def test_rng_restatement_equals_softmax_dropout(cuda):
    """Attention counter layout (st5_softmax_fwd's dropped probabilities), S > 64, lds = ceil8(S) != S, bit for bit."""
    BH, H, T, S, p, seed = 24, 12, 70, 100, 0.1, 55555
    lds = 104
    scores = (torch.randn(BH, T, lds) * 0.5).to(cuda)
    probs = torch.full((BH, T, lds), float("nan"), device=cuda)
    pdrop = torch.full((BH, T, lds), float("nan"), device=cuda)
    hip.check(hip.lib().st5_softmax_fwd(scores.data_ptr(), hip.ptr(None), hip.ptr(None), probs.data_ptr(), pdrop.data_ptr(), BH, H, T, S, lds, 0, 0, 0,
                                        p, seed, hip.F32, hip.stream()), "st5_softmax_fwd")
    pd = pdrop[:, :, :S].cpu()
    assert torch.all(probs[:, :, :S].cpu() > 0)
    assert np.array_equal((pd != 0).numpy(), R.keep_mask_attention(seed, p, BH, T, S))


# ---- the unfused bf16 path with probabilities (TTS guided attention) -----------------------------------------------------
UNFUSED_BAR = 2.0 ** -5   # scores, probabilities, dP and dS all pass through bf16 buffers on this path (measured worst rows 0.008-0.013)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_unfused_attention_with_probs_tts_cross(cuda, p, monkeypatch):
    B, H, T, S = 4, 12, 300, 100
    d = H * HD
    g = torch.Generator().manual_seed(77 + int(10 * p))
    xq = _bf(torch.randn(B * T, d, generator=g))
    xkv = _bf(torch.randn(B * S, 2 * d, generator=g))
    dout = _bf(torch.randn(B * T, d, generator=g))
    gp = torch.randn(B, H, T, S, generator=g) * 0.05
    kpm = _kpm(B, S, [100, 87, 64, 1])
    seed = SEED + 99
    monkeypatch.setattr(Fn, "next_seed", lambda: seed)
    Fn.set_compute_dtype(torch.bfloat16)
    try:
        XQ = xq.to(cuda).requires_grad_(True)
        XKV = xkv.to(cuda).requires_grad_(True)
        with poisoned_allocations():
            ctx, probs = Fn.CrossAttentionFunction.apply(XQ, XKV, kpm.to(cuda), (B, H, T, S, HD, p, True))
            ((ctx.float() * dout.to(cuda).float()).sum() + (probs * gp.to(cuda)).sum()).backward()
        torch.cuda.synchronize()
    finally:
        Fn.set_compute_dtype(torch.float32)
    keep = (lambda bh: R.keep_mask_attention(seed, p, B * H, T, S, rows=[bh])[0]) if p > 0 else None
    ref = R.attention_fwd_bwd_fp64(_heads(xq, B, T, H), _heads(xkv, B, S, H), _heads(xkv, B, S, H, d), _heads(dout, B, T, H),
                                   None, 0, kpm, False, keep, p, dprobs=gp.double())
    got = dict(o=_heads(ctx.detach(), B, T, H), probs=probs.detach().double().cpu(), dq=_heads(XQ.grad, B, T, H),
               dk=_heads(XKV.grad, B, S, H), dv=_heads(XKV.grad, B, S, H, d))
    for nm, t in got.items():
        assert torch.isfinite(t).all(), nm
        err = row_metric(t, ref[nm])
        print(f"attention fp64 pin: unfused p={p}: {nm} worst row {err:.3e}")
        assert err <= UNFUSED_BAR, f"unfused {nm}: worst row {err:.3e}"
