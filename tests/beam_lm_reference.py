"""fp64 restatement of st5_beam_lm_logprobs (csrc/beam_lm.hip) in plain torch: the LM term of a device-stepped beam search step.

Both forms take the values the kernel reads (fp32 decoder logits or log-probabilities, LM logits in fp32 or bf16) and compute in fp64:
  logits form:    lp[r][c] = x[r][c] / T - max_c - log(sum_c exp(x[r][c] / T - max_c)), then for c < V_lm
                  lp[r][c] += w * (y[r][c] - max_lm - log(sum exp(y[r] - max_lm)));
  in-place form:  the LM term alone, added into given log-probabilities.
A row with a NaN decoder logit is NaN throughout (the kernel's sum of exponentials is); -inf stays -inf; columns V_lm .. V - 1 get no
LM term.  `gated`: a counter outside [0, max_len] writes nothing (the caller's buffer is returned unchanged)."""
import torch


def lm_term(lm_logits, w):
    """w * log_softmax(lm_logits) in fp64, row by row with the maximum taken out first."""
    y = lm_logits.double()
    mx = y.max(dim=-1, keepdim=True).values
    lse = torch.log(torch.exp(y - mx).sum(dim=-1, keepdim=True))
    return float(w) * ((y - mx) - lse)


def log_probs(logits, temperature):
    """The unruled log-softmax of logits / temperature in fp64 (NaN rows stay NaN: torch.max propagates it, as the kernel's sum does)."""
    x = logits.double() / float(temperature)
    mx = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x).max(dim=-1, keepdim=True).values
    lse = torch.log(torch.exp(x - mx).sum(dim=-1, keepdim=True))
    return (x - mx) - lse


def fuse_logits(logits, V, temperature, lm_logits, w):
    """The logits form: fp64 [rows, V] from logits [rows, >= V] (columns past V are never read) and lm_logits [rows, V_lm]."""
    lp = log_probs(logits[:, :V], temperature)
    V_lm = lm_logits.shape[1]
    assert V_lm <= V
    lp[:, :V_lm] = lp[:, :V_lm] + lm_term(lm_logits, w)
    return lp


def fuse_in_place(lp, V, lm_logits, w):
    """The in-place form: fp64 [rows, V] from log-probabilities lp [rows, >= V] (the CTC-mixed ones)."""
    out = lp[:, :V].double().clone()
    V_lm = lm_logits.shape[1]
    assert V_lm <= V
    out[:, :V_lm] = out[:, :V_lm] + lm_term(lm_logits, w)
    return out
