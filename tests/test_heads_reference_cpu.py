"""Pins the fp64 restatements in tests/heads_reference.py to the oracle functions they restate, on small inputs, values and
gradients: vq_restated to oracle.gumbel_quantizer (identity weight_proj), nce_restated to oracle.hubert_logits (identity
final_proj).  tests/test_heads_gpu.py holds st5_vq_*, st5_nce_logits*, st5_canon_rows and st5_norm_rows* to these restatements."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from oracle import speecht5_oracle as O
from tests.heads_reference import nce_restated, vq_restated

D64 = torch.float64


def _close(a, b, tol):
    """max |a - b| <= tol * max |b| over the finite entries, with the same non-finite pattern (the oracle computes in fp32 where
    the reference casts with .float(), so the bars are fp32 ones)."""
    a, b = a.double(), b.double()
    assert a.shape == b.shape
    assert torch.equal(torch.isfinite(a), torch.isfinite(b))
    fin = torch.isfinite(b)
    scale = max(float(b[fin].abs().max()), 1e-30) if fin.any() else 1.0
    assert float((a[fin] - b[fin]).abs().max()) <= tol * scale if fin.any() else True


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("G,V", [(2, 10), (1, 7), (2, 100)])
def test_vq_restatement_matches_oracle(G, V, training):
    gen = torch.Generator().manual_seed(11 * G + V + int(training))
    B, T, Dg, tau, c = 3, 5, 4, 0.5, -0.3
    C = G * V
    x = torch.randn(B, T, C, generator=gen, dtype=D64)
    x[0, 1, 0] = x[0, 1, V - 1] = 9.0                     # an exact tie in group 0: the lower index wins in both
    vars_ = torch.rand(1, C, Dg, generator=gen, dtype=D64)
    noise = -torch.empty(B * T * G, V, dtype=D64).exponential_(generator=gen).log() if training else None
    if training:
        noise[G, 0] = noise[G, V - 1] = 0.0
    sd = {"quantizer.weight_proj.weight": torch.eye(C, dtype=D64), "quantizer.weight_proj.bias": torch.zeros(C, dtype=D64),
          "quantizer.vars": vars_}
    xo, xr = x.clone().requires_grad_(), x.clone().requires_grad_()
    ref = O.gumbel_quantizer(sd, SimpleNamespace(latent_groups=G, latent_vars=V), xo, gumbel_noise=noise, tau=tau)
    got = vq_restated(xr.view(B * T, C), vars_.view(C, Dg), G, V, gumbel=None if noise is None else noise.view(B * T, C), tau=tau)
    assert int(got["idx"][1, 0]) == 0
    _close(got["out"].view(B, T, -1).detach(), ref["x"].detach(), 1e-6)
    _close(got["code_perplexity"].detach(), ref["code_perplexity"].detach(), 1e-6)
    _close(got["prob_perplexity"].detach(), ref["prob_perplexity"].detach(), 1e-6)
    dout = torch.randn(B, T, G * Dg, generator=gen, dtype=D64)
    (go,) = torch.autograd.grad((ref["x"] * dout).sum() + c * ref["prob_perplexity"], xo)
    (gr,) = torch.autograd.grad((got["out"].view(B, T, -1) * dout).sum() + c * got["prob_perplexity"], xr)
    _close(gr, go, 1e-5)
    # handed the mean softmax it computes itself, the avg= form is the same function with the same gradient
    xa = x.clone().requires_grad_()
    same = vq_restated(xa.view(B * T, C), vars_.view(C, Dg), G, V, gumbel=None if noise is None else noise.view(B * T, C), tau=tau,
                       avg=got["avg"].detach())
    (ga,) = torch.autograd.grad((same["out"].view(B, T, -1) * dout).sum() + c * same["prob_perplexity"], xa)
    assert torch.equal(same["prob_perplexity"], got["prob_perplexity"]) and torch.allclose(ga, gr, rtol=1e-12, atol=0)


@pytest.mark.parametrize("S,V,D", [(7, 9, 5), (23, 20, 8)])
def test_nce_restatement_matches_oracle(S, V, D):
    gen = torch.Generator().manual_seed(S * V + D)
    temp = 0.1
    emb = torch.randn(V, D, generator=gen, dtype=D64)
    emb[4] = emb[1]                                     # bitwise duplicate
    emb[6] = 0.0                                        # all-zero row
    emb[7, 0] = 0.0
    emb[8] = emb[7]
    emb[8, 0] = -0.0                                    # equal to row 7 under ==, not bitwise
    x = torch.randn(S, D, generator=gen, dtype=D64)
    x[2] = 0.0
    x[3] *= 1e15
    tgt = torch.randint(0, V, (S,), generator=gen)
    tgt[:5] = torch.tensor([1, 4, 6, 8, 7])
    eo, er = emb.clone().requires_grad_(), emb.clone().requires_grad_()
    xo, xr = x.clone().requires_grad_(), x.clone().requires_grad_()
    sd = {"hubert_layer.label_embs_concat": eo, "hubert_layer.final_proj.weight": torch.eye(D, dtype=D64),
          "hubert_layer.final_proj.bias": torch.zeros(D, dtype=D64)}
    ref, _ = O.hubert_logits(sd, SimpleNamespace(logit_temp=temp), xo.view(1, S, D), torch.zeros(1, S, dtype=torch.bool),
                             torch.ones(1, S, dtype=torch.bool), [tgt.view(1, S)])
    got = nce_restated(xr, er, tgt, temp)
    assert int(torch.isinf(got).sum()) > S                # the duplicate classes are masked beside each positive's own
    _close(got.detach(), ref.detach(), 1e-6)
    zero = torch.zeros(S, dtype=torch.long)
    gxo, geo = torch.autograd.grad(F.cross_entropy(ref, zero, reduction="sum"), [xo, eo])
    gxr, ger = torch.autograd.grad(F.cross_entropy(got, zero, reduction="sum"), [xr, er])
    for rows in (torch.arange(S) != 2, torch.arange(S) == 2):     # the zero row's gradient is 1 / eps larger
        _close(gxr[rows], gxo[rows], 1e-5)
    for rows in (torch.arange(V) != 6, torch.arange(V) == 6):
        _close(ger[rows], geo[rows], 1e-5)
