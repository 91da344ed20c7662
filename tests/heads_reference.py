"""fp64 restatements of the three pre-training heads at the logits level, the references tests/test_heads_gpu.py holds the HIP
kernels to.  tests/test_heads_reference_cpu.py pins each one to the oracle function it restates (oracle/speecht5_oracle.py), so
they stand on the goldens rather than on their own reading of the reference."""
import torch
import torch.nn.functional as F

PERP_EPS = 1e-7   # fairseq GumbelVectorQuantizer: log(p + 1e-7)
NORM_EPS = 1e-8   # torch.cosine_similarity's eps


def vq_restated(logits, vars_, G, V, gumbel=None, tau=2.0, idx=None, enc=None, mix_w=None, T=1, avg=None):
    """oracle.gumbel_quantizer after its weight_proj, plus the time-wise mix: logits [N, G*V], vars_ [G*V, Dg], gumbel [N, G*V]
    (None: eval, the hard arg-max).  `idx` [N, G] (within-group index) overrides the selection the arg-max would make, so a
    caller can evaluate the straight-through gradient at the selection the kernel made.  mix_w [T]: out[n] = w q + (1 - w) enc
    with w = mix_w[n % T].  `avg` [G, V]: the mean softmax at which prob_perplexity and its gradient are evaluated (default: the
    one computed here), so that a caller can state the gradient a backward pass owes for the mean it was handed; the gradient
    still flows through the softmax of `logits`.  Returns dict(out [N, G*Dg], code_perplexity, prob_perplexity, avg [G, V],
    idx [N, G])."""
    N = logits.shape[0]
    lg = logits.view(N, G, V)
    k = lg.argmax(-1)
    hp = F.one_hot(k, V).to(logits.dtype).mean(0)
    code_ppl = torch.exp(-torch.sum(hp * torch.log(hp + PERP_EPS), dim=-1)).sum()
    ap = torch.softmax(lg, dim=-1).mean(0)
    if avg is not None:
        ap = ap + (avg.to(ap.dtype) - ap).detach()
    prob_ppl = torch.exp(-torch.sum(ap * torch.log(ap + PERP_EPS), dim=-1)).sum()
    if gumbel is not None:   # F.gumbel_softmax(hard=True) with the given noise: hard one-hot forward, soft gradient
        y = ((lg + gumbel.view(N, G, V)) / tau).softmax(-1)
        sel_i = y.argmax(-1) if idx is None else idx
        sel = F.one_hot(sel_i, V).to(y.dtype) - y.detach() + y
    else:
        sel_i = k if idx is None else idx
        sel = F.one_hot(sel_i, V).to(logits.dtype)
    q = torch.einsum("ngv,gvd->ngd", sel, vars_.view(G, V, -1)).reshape(N, -1)
    if mix_w is not None:
        w = mix_w.repeat(N // T)[:, None]
        q = w * q + (1 - w) * enc
    return dict(out=q, code_perplexity=code_ppl, prob_perplexity=prob_ppl, avg=ap, idx=sel_i)


def same_rows(emb):
    """[V, V] bool: row c equals row c' element-wise under == (so -0.0 equals +0.0), the reference's neg_is_pos test."""
    return (emb[:, None, :] == emb[None, :, :]).all(-1)


def nce_restated(x, emb, target, temp):
    """oracle.hubert_logits' nce() without its [1 + V, S, D] comparison tensor: cosine similarities as one product of rows
    scaled to unit length (norms clamped at eps as torch.cosine_similarity clamps them), the positive first, then every class,
    -inf at each class whose code-book row equals the positive's row.  x [S, D], emb [V, D], target [S] -> [S, 1 + V]."""
    xn = x / x.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS)
    en = emb / emb.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS)
    sim = xn @ en.t()
    t = target.long()
    pos = sim.gather(1, t.view(-1, 1))
    neg = sim.masked_fill(same_rows(emb)[t], float("-inf"))
    return torch.cat([pos, neg], dim=1) / temp
