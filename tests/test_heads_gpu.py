"""Kernel-level tests of the three heads of the speech + text pre-training step, each against a plain fp64 reference on CPU
evaluated on exactly the inputs the kernel sees (the same fp32 logits, bf16 values after their rounding):

- Gumbel vector quantiser, functional.GumbelVQFunction: st5_vq_fwd (vq_fwd_kernel + vq_final_kernel), the batched dsel GEMM,
  st5_vq_bwd, st5_embed_rows_bwd_det_w.  Shapes with several rows per wave, with live lanes in the second half of the wave
  (V > 64), V = VP = 128 with idle trailing waves (2048 waves, G = 3), exact ties within and across the wave halves.
- HuBERT NCE head, functional.NCELogitsFunction: st5_norm_rows, st5_canon_rows, the cosine GEMM, st5_nce_logits,
  st5_nce_logits_bwd, st5_norm_rows_bwd.  Code books with bitwise-duplicate rows, a -0.0 / +0.0 pair, an all-zero row;
  x rows of zero norm and of magnitude ~1e15; S = 0; class counts 504 (km500 + 4 specials), 100 and 54 (not a multiple of 4).
- Masked Tacotron loss, functional.tacotron_loss: st5_tacotron_loss_fwd, st5_tacotron_loss_bwd.  r = 1 / 2 / 3, lengths that
  are not multiples of r, one frame left after the trim, ys / labels with a batch stride wider than L, logits up to +-80.

The references (tests/heads_reference.py, oracle.tacotron_loss) are pinned to the oracle by tests/test_heads_reference_cpu.py.
Every buffer the product allocates is poisoned first (tests.util.poisoned_allocations) and strided inputs carry NaN in their
gaps and in masked frames, so a read of memory nobody wrote shows up as NaN."""
import pytest
import torch
import torch.nn.functional as F

from oracle import speecht5_oracle as O
from speecht5_amd import functional as Fn
from speecht5_amd import hip
from speecht5_amd.modules.gumbel_vector_quantizer import GumbelVectorQuantizer
from tests.heads_reference import nce_restated, same_rows, vq_restated
from tests.util import poisoned_allocations

pytestmark = pytest.mark.gpu

D64 = torch.float64


def rel_fro(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def rel_max(got, ref, unit=0.0):
    """max |got - ref| / max(max |ref|, unit); an all-zero reference (and unit) demands an all-zero result."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all()
    err, scale = float((got - ref).abs().max()), max(float(ref.abs().max()), unit)
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


def outputs_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b) if x is not None)


# ------------------------------------------------------------------------------------------------------------------------------
# Gumbel vector quantiser
# ------------------------------------------------------------------------------------------------------------------------------
# (N, G, V, Dg, T): N rows = B x T frames; T is the mix period
VQ_SHAPES = [(3992, 2, 100, 384, 499), (998, 2, 100, 384, 499), (8192, 2, 100, 384, 512), (37, 2, 64, 384, 37),
             (517, 2, 65, 8, 47), (2049, 3, 128, 96, 683), (5, 1, 10, 8, 5)]
# (training, tau, tau as a device tensor, 0/1 time-wise mix)
VQ_MODES = [(False, 2.0, False, False), (False, 0.5, True, True), (True, 2.0, False, True), (True, 0.5, True, False),
            (True, 0.5, False, True), (True, 2.0, True, False)]


def _mode_id(m):
    return ("train" if m[0] else "eval") + f"-tau{m[1]}" + ("dev" if m[2] else "") + ("-mix" if m[3] else "")


def _tie_pairs(V):
    """(a, b) pairs of equal maxima: within the first half-wave, and across the halves (lane v and v + 64) where V allows."""
    pairs = [(3, min(40, V - 1))]
    if V > 64:
        pairs.append((3, 67 if V > 67 else 64))
    return pairs


@pytest.mark.parametrize("mode", VQ_MODES, ids=_mode_id)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", VQ_SHAPES, ids=lambda s: "N{}-G{}-V{}-Dg{}".format(*s[:4]))
def test_gumbel_vq(cuda, shape, dtype, mode):
    """st5_vq_fwd / st5_vq_bwd / st5_embed_rows_bwd_det_w through GumbelVQFunction against the fp64 straight-through
    restatement of oracle.gumbel_quantizer."""
    N, G, V, Dg, T = shape
    training, tau, tau_on_dev, mixed = mode
    seed = (N * 7 + G * 131 + V * 17 + Dg) * 8 + training * 4 + tau_on_dev * 2 + mixed
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, G * V, generator=gen) * 1.5
    vars_ = torch.rand(G * V, Dg, generator=gen)
    dout = torch.randn(N, G * Dg, generator=gen).to(dtype)
    enc = torch.randn(N, G * Dg, generator=gen).to(dtype) if mixed else None
    mix_w = None
    if mixed:
        mix_w = (torch.rand(T, generator=gen) < 0.5).float()
        mix_w[0], mix_w[-1] = 1.0, 0.0
    grad0 = torch.randn(G * V, Dg, generator=gen)
    c = -0.7 / (G * V)        # d loss / d prob_perplexity of the criterion's (num_vars - prob_ppl) / num_vars term, weighted
    torch.manual_seed(seed)
    gum = GumbelVectorQuantizer.gumbel_noise(None, logits.to(cuda)).cpu() if training else None
    # exact ties in the hard logits (and in the noisy ones), within one half-wave and across the halves
    tie_rows = torch.arange(1, N, 97)
    tie_at = {}
    for j, n in enumerate(tie_rows.tolist()):
        g = j % G
        a, b = _tie_pairs(V)[j % len(_tie_pairs(V))]
        logits[n, g * V + a] = logits[n, g * V + b] = 30.0
        if training:
            gum[n, g * V + a] = gum[n, g * V + b] = 0.0
        tie_at[(n, g)] = a

    def run():
        lg = logits.to(cuda).requires_grad_()
        vp = vars_.view(1, G * V, Dg).to(cuda).requires_grad_()
        vp.grad = grad0.view(1, G * V, Dg).to(cuda)
        vc = vp.detach().view(G * V, Dg).to(dtype)
        e = enc.to(cuda).requires_grad_() if mixed else None
        t = torch.tensor([tau], dtype=torch.float32, device=cuda) if tau_on_dev else tau
        with poisoned_allocations():
            out, code_pp, prob_pp, idx = Fn.GumbelVQFunction.apply(lg, vp, vc, e, gum.to(cuda) if training else None,
                                                                   mix_w.to(cuda) if mixed else None, t, training, G, V, T, dtype)
            avg = out.grad_fn.saved_tensors[3].clone()
            torch.autograd.backward([out, prob_pp], [dout.to(cuda), torch.tensor(c, device=cuda)])
        torch.cuda.synchronize()
        return [x.detach().cpu() if x is not None else None
                for x in (out, code_pp, prob_pp, idx, avg, lg.grad, vp.grad.view(G * V, Dg), e.grad if mixed else None)]

    r1 = run()
    out, code_pp, prob_pp, idx, avg, dlogits, dvars, denc = r1
    # selection: the kernel's own fp32 expression, arg-max with the lowest index on ties (torch.argmax on CPU)
    if training:
        z = (logits + gum) * (torch.tensor(1.0) / torch.tensor(tau, dtype=torch.float32))
        want = z.view(N, G, V).argmax(-1)
    else:
        want = logits.view(N, G, V).argmax(-1)
    assert torch.equal(idx.long(), want + torch.arange(G) * V), "code rows"
    for (n, g), a in tie_at.items():
        assert int(want[n, g]) == a
    # ... and the fp64 arg-max of the softmax wherever its top-two gap is resolvable in fp32
    z64 = (logits.double() + gum.double()) / tau if training else logits.double()
    top = z64.view(N, G, V).topk(2, dim=-1).values
    clear = (top[..., 0] - top[..., 1]) > 1e-5 * top[..., 0].abs()
    tied = torch.zeros(N, G, dtype=torch.bool)
    for (n, g) in tie_at:
        tied[n, g] = True
    assert torch.equal(z64.view(N, G, V).argmax(-1)[clear], want[clear])
    excluded = int((~clear & ~tied).sum())
    print(f"vq {shape} {_mode_id(mode)}: {excluded} of {N * G} selections excluded from the fp64 arg-max comparison")
    assert excluded < 1e-3 * N * G
    # forward
    q = vars_.view(G, V, Dg)[torch.arange(G), want].reshape(N, G * Dg)
    if mixed:
        wrow = mix_w.repeat(N // T)[:, None]
        q = torch.where(wrow == 1.0, q, enc.float())
    assert torch.equal(out, q.to(dtype)), "out"
    l64 = logits.double().requires_grad_()
    ref = vq_restated(l64, vars_.to(dtype).double(), G, V, gumbel=gum.double() if training else None, tau=tau, idx=want,
                      enc=enc.double() if mixed else None, mix_w=mix_w.double() if mixed else None, T=T)
    assert float((avg[:, :V].double() - ref["avg"].detach()).abs().max()) <= 1e-6
    assert torch.equal(avg[:, V:], torch.zeros(G, avg.shape[1] - V))
    assert abs(float(code_pp) - float(ref["code_perplexity"])) <= 1e-6 * float(ref["code_perplexity"])
    assert abs(float(prob_pp) - float(ref["prob_perplexity"].detach())) <= 1e-5 * float(ref["prob_perplexity"].detach())
    # backward: loss = <dOut, out> + c * prob_perplexity.  st5_vq_bwd is handed the forward's mean softmax `avg` (held to fp64
    # above), and the perplexity gradient differences log(avg) across a near-uniform code book, which scales avg's fp32
    # rounding up ~10x; so the fp64 gradient is evaluated at the avg the backward was handed, like every other input it sees.
    l64 = logits.double().requires_grad_()
    ref = vq_restated(l64, vars_.to(dtype).double(), G, V, gumbel=gum.double() if training else None, tau=tau, idx=want,
                      enc=enc.double() if mixed else None, mix_w=mix_w.double() if mixed else None, T=T, avg=avg[:, :V].double())
    ((ref["out"] * dout.double()).sum() + c * ref["prob_perplexity"]).backward()
    tol = 1e-5 if dtype == torch.float32 else 2e-3
    assert rel_fro(dlogits, l64.grad) <= tol, "dlogits"
    w_n = mix_w.repeat(N // T)[:, None] if mixed else torch.ones(N, 1)
    if mixed:
        assert torch.equal(denc, ((1.0 - w_n) * dout.float()).to(dtype)), "denc"
    rows = (want + torch.arange(G) * V).reshape(-1)
    dv = torch.zeros(G * V, Dg, dtype=D64).index_add_(0, rows, (w_n * dout.double()).view(N, G, Dg).reshape(N * G, Dg))
    assert rel_fro(dvars, grad0.double() + dv) <= 1e-5, "dvars"
    assert outputs_equal(r1, run()), "two runs differ"


# ------------------------------------------------------------------------------------------------------------------------------
# HuBERT NCE head
# ------------------------------------------------------------------------------------------------------------------------------
ROW0 = 2            # the head's classes are rows ROW0 .. ROW0 + V - 1 of the shared code-book parameter
DUPS = (5, 17, 9)   # bitwise-equal rows
ZERO_ROW = 30
PM0 = (40, 41)      # equal under ==, one holds -0.0 where the other holds +0.0


def _nce_inputs(S, V, D, xdtype, gen):
    emb = torch.randn(V + ROW0 + 3, D, generator=gen)
    r = lambda c: ROW0 + c  # noqa: E731
    emb[r(DUPS[1])] = emb[r(DUPS[0])]
    emb[r(DUPS[2])] = emb[r(DUPS[0])]
    emb[r(ZERO_ROW)] = 0.0
    emb[r(PM0[0]), 0] = 0.0
    emb[r(PM0[1])] = emb[r(PM0[0])]
    emb[r(PM0[1]), 0] = -0.0
    x = torch.randn(S, D, generator=gen)
    x[3::50] = 0.0
    x[4::50] *= 1e15
    tgt = torch.randint(0, V, (S,), generator=gen)
    hit = torch.tensor(DUPS + (ZERO_ROW,) + PM0)
    k = torch.arange(0, S, 7)
    tgt[k] = hit[torch.arange(k.numel()) % hit.numel()]
    return emb, x.to(xdtype), tgt


def _x_groups(S):
    s = torch.arange(S)
    return {"zero-norm": s % 50 == 3, "1e15": s % 50 == 4, "other": (s % 50 != 3) & (s % 50 != 4)}


NCE_DX = [(256, torch.float32), (768, torch.bfloat16), (768, torch.float32)]


@pytest.mark.parametrize("D,xdtype", NCE_DX, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("V", [504, 100, 54])
@pytest.mark.parametrize("S", [0, 1, 37, 2000, 3992])
def test_nce_head(cuda, S, V, D, xdtype):
    """st5_norm_rows / st5_canon_rows / st5_nce_logits / st5_nce_logits_bwd / st5_norm_rows_bwd through NCELogitsFunction against
    the fp64 restatement of oracle.hubert_logits, with the speech_pretrain_loss upstream (cross entropy to class 0, summed)."""
    temp = 0.1
    gen = torch.Generator().manual_seed(S * 1009 + V * 7 + D)
    emb, x, tgt = _nce_inputs(S, V, D, xdtype, gen)
    x64 = x.double().requires_grad_()
    e64 = emb[ROW0:ROW0 + V].double().requires_grad_()
    ref = nce_restated(x64, e64, tgt, temp)
    if S > 0:
        F.cross_entropy(ref, torch.zeros(S, dtype=torch.long), reduction="sum").backward()
    de = e64.grad if S > 0 else torch.zeros(V, D, dtype=D64)
    grad0 = torch.randn(emb.shape, generator=gen, dtype=D64) * max(float(de[torch.arange(V) != ZERO_ROW].pow(2).mean().sqrt()), 1e-3)
    grad0 = grad0.float()

    def run():
        xd = x.to(cuda).requires_grad_()
        ep = emb.to(cuda).requires_grad_()
        ep.grad = grad0.to(cuda)
        with poisoned_allocations():
            logits = Fn.NCELogitsFunction.apply(xd, ep, ROW0, V, tgt.to(cuda), temp)
            F.cross_entropy(logits, torch.zeros(S, dtype=torch.long, device=cuda), reduction="sum").backward()
        torch.cuda.synchronize()
        return [logits.detach().cpu(), xd.grad.cpu() if xd.grad is not None else None, ep.grad.cpu()]

    r1 = run()
    logits, dx, demb = r1
    assert logits.shape == (S, V + 1)
    if S == 0:
        assert torch.equal(demb, grad0), "S = 0 touched the code-book gradient"
        assert dx is None or dx.shape == (0, D)
        return
    # forward: the same -inf set, finite logits within 1e-5 / temp
    assert not torch.isnan(logits).any()
    assert torch.equal(torch.isinf(logits), torch.isinf(ref.detach())), "-inf positions"
    fin = torch.isfinite(ref.detach())
    assert float((logits.double()[fin] - ref.detach()[fin]).abs().max()) <= 1e-5 / temp
    # every class equal to the positive's row is masked: duplicates, the -0.0 / +0.0 pair
    assert torch.isinf(logits[:, 1:][same_rows(emb[ROW0:ROW0 + V])[tgt]]).all()
    # backward
    tol = 1e-5 if xdtype == torch.float32 else 2e-3
    for name, m in _x_groups(S).items():
        if m.any():
            assert rel_fro(dx[m], x64.grad[m]) <= tol, f"dx ({name} rows)"
    want = grad0.double()
    want[ROW0:ROW0 + V] += de
    inside = torch.zeros(emb.shape[0], dtype=torch.bool)
    inside[ROW0:ROW0 + V] = True
    assert torch.equal(demb[~inside], grad0[~inside]), "rows outside the head's classes"
    zr = torch.zeros_like(inside)
    zr[ROW0 + ZERO_ROW] = True
    for name, m in (("zero row", zr), ("other rows", inside & ~zr)):
        assert rel_fro(demb[m], want[m]) <= 1e-5, f"code-book gradient ({name})"
    assert outputs_equal(r1, run()), "two runs differ"


@pytest.mark.parametrize("V", [504, 100, 54])
def test_nce_logits_bwd_masks_duplicate_classes(cuda, V):
    """st5_nce_logits_bwd on its own (the Function's upstream is already zero at -inf classes): an upstream that is non-zero
    everywhere must give dsim = 0 at every class equal to the positive's row except the positive's own column, which takes
    the positive logit's gradient; the padding columns of a row stride rounded up to 4 are written as 0."""
    S, D, temp = 300, 16, 0.1
    gen = torch.Generator().manual_seed(V)
    emb, _, tgt = _nce_inputs(S, V, D, torch.float32, gen)
    e = emb[ROW0:ROW0 + V].contiguous()
    g = torch.randn(S, V + 1, generator=gen)
    ld = (V + 3) // 4 * 4 + 4
    L = hip.lib()
    with poisoned_allocations():
        canon = torch.empty(V, dtype=torch.int32, device=cuda)
        dsim = torch.empty(S, ld, dtype=torch.float32, device=cuda)
        ed, gd, td = e.to(cuda), g.to(cuda), tgt.to(torch.int32).to(cuda)
        hip.check(L.st5_canon_rows(ed.data_ptr(), canon.data_ptr(), V, D, hip.stream()), "st5_canon_rows")
        hip.check(L.st5_nce_logits_bwd(gd.data_ptr(), td.data_ptr(), canon.data_ptr(), dsim.data_ptr(), ld, S, V, temp, hip.stream()),
                  "st5_nce_logits_bwd")
    torch.cuda.synchronize()
    same = same_rows(e)
    want_canon = torch.tensor([int(same[c].nonzero()[0]) for c in range(V)], dtype=torch.int32)
    assert torch.equal(canon.cpu(), want_canon)
    inv_t = torch.tensor(1.0) / torch.tensor(temp, dtype=torch.float32)
    want = torch.where(same[tgt], torch.zeros(()), g[:, 1:] * inv_t)
    want[torch.arange(S), tgt] += g[:, 0] * inv_t
    got = dsim.cpu()
    assert torch.equal(got[:, :V], want)
    assert torch.equal(got[:, V:], torch.zeros(S, ld - V))


# ------------------------------------------------------------------------------------------------------------------------------
# Masked Tacotron loss
# ------------------------------------------------------------------------------------------------------------------------------
def _olens(B, L, r, gen):
    """untrimmed lengths in [r, L]: L itself, r (one frame left after the trim), one that is not a multiple of r, then random."""
    odd = next(v for v in range(L - 1, 0, -1) if v % r != 0) if r > 1 else L - 1
    cand = [L, r, odd]
    if B == 1:
        return torch.tensor([cand[r % len(cand)]])
    rest = torch.randint(r, L + 1, (max(B - len(cand), 0),), generator=gen)
    return torch.cat([torch.tensor(cand[:B]), rest])


@pytest.mark.parametrize("pw", [5.0, 1.0])
@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("L", [7, 626, 1000])
@pytest.mark.parametrize("B", [1, 8, 32])
def test_tacotron_loss(cuda, B, L, r, pw):
    """st5_tacotron_loss_fwd / st5_tacotron_loss_bwd through Fn.tacotron_loss against oracle.tacotron_loss in fp64."""
    C = 80
    gen = torch.Generator().manual_seed(B * 100003 + L * 31 + r * 7 + int(pw))
    olens = _olens(B, L, r, gen)
    eff = olens - olens % r
    valid = torch.arange(L)[None, :] < eff[:, None]                          # [B, L]
    after = torch.randn(B, L, C, generator=gen)
    before = torch.randn(B, L, C, generator=gen)
    logits = (torch.rand(B, L, generator=gen) * 2 - 1) * 80.0
    ys_full = torch.randn(B, L + 3, C, generator=gen)
    lab_full = (torch.rand(B, L + 5, generator=gen) < 0.1).float()
    # NaN wherever the kernel must not read: masked frames, the gaps of the wider batch strides
    for t in (after, before, ys_full[:, :L]):
        t[~valid] = float("nan")
    logits[~valid] = float("nan")
    lab_full[:, :L][~valid] = float("nan")
    ys_full[:, L:] = float("nan")
    lab_full[:, L:] = float("nan")
    ys, labels = ys_full[:, :L], lab_full[:, :L]

    # fp64 oracle
    a64, b64, l64 = (t.double().requires_grad_() for t in (after, before, logits))
    mx = int(eff.max()) if r > 1 else L
    sample = {"dec_target": ys.double(), "labels": labels.double(), "dec_target_lengths": olens}
    _, rl1, rl2, rbce = O.tacotron_loss(b64[:, :mx], a64[:, :mx], l64[:, :mx], sample, r, bce_pos_weight=pw)

    def run(patterns):
        ad, bd, ld = (t.to(cuda).requires_grad_() for t in (after, before, logits))
        ysd, labd = ys_full.to(cuda)[:, :L], lab_full.to(cuda)[:, :L]
        assert ysd.stride(0) > L * C and labd.stride(0) > L
        res = []
        with poisoned_allocations():
            l1, mse, bce = Fn.tacotron_loss(ad, bd, ld, ysd, labd, olens.to(cuda), r, pw)
            res.append(torch.stack([l1, mse, bce]).detach().cpu())
            for gs in patterns:
                gd = [torch.tensor(v, dtype=torch.float32, device=cuda) for v in gs]
                res.append([d.cpu() for d in torch.autograd.grad([l1, mse, bce], [ad, bd, ld], gd, retain_graph=True)])
        torch.cuda.synchronize()
        return res

    rnd = tuple(float(v) for v in torch.randn(3, generator=gen))
    patterns = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), rnd]
    r1 = run(patterns)
    got = r1[0].double()
    for k, (name, want) in enumerate((("l1", rl1), ("mse", rl2), ("bce", rbce))):
        assert abs(float(got[k]) - float(want)) <= 1e-6 * abs(float(want)), name
    for gs, grads in zip(patterns, r1[1:]):
        want = torch.autograd.grad(gs[0] * rl1 + gs[1] * rl2 + gs[2] * rbce, [a64, b64, l64], retain_graph=True)
        for name, g, w in zip(("d_after", "d_before", "d_logits"), grads, want):
            assert (g[~valid] == 0).all(), f"{name} {gs}: masked positions"
            # d_logits is relative to its unit |g3| max(1, pw) / n_frames: where the only valid frame has a label of 1 and a
            # logit of +80, its exact value pw (sigmoid(x) - 1) ~ 1e-35 is below what fp32 resolves next to the unit
            unit = abs(gs[2]) * max(1.0, pw) / float(eff.sum()) if name == "d_logits" else 0.0
            assert rel_max(g, w, unit) <= 1e-6, f"{name} {gs}"
    r2 = run(patterns[3:])
    assert torch.equal(r1[0], r2[0]) and all(torch.equal(a, b) for a, b in zip(r1[4], r2[1])), "two runs differ"
