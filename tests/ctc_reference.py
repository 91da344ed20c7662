"""Plain references of the two CTC kernels, the yardsticks tests/test_ctc_gpu.py and tests/test_generator_gpu.py hold them to:

- ctc_loss_ref: torch's own CTC (F.ctc_loss, the recursion the reference criterion runs with cuDNN off) on CPU in a chosen
  precision, evaluated at exactly the fp32 log-probabilities the kernel saw.  fp64 is the reference; fp32 measures what fp32
  log-space alpha / beta rows cost on their own, the error model the kernel's error is judged by.
- prefix_initial / prefix_score: the prefix-score recursion of joint CTC / attention beam search (espnet CTCPrefixScore, in-tree
  copy Speech2C/speech2c/models/modules/ctc_prefix_score.py:10-112) in numpy, in any float dtype: float32 restates the
  reference's arithmetic, float64 is the reference, with the same LOGZERO = -1e10 sentinel and start = max(out_len, 1) rule.

tests/test_ctc_reference_cpu.py pins both to brute-force sums over every alignment of small cases."""
import numpy as np
import torch
import torch.nn.functional as F

LOGZERO = -1e10   # ctc_prefix_score.py:21


def ctc_loss_ref(lprobs, targets, input_lengths, target_lengths, blank, zero_infinity, grad_out=1.0, logits=None,
                 dtype=torch.float64):
    """F.ctc_loss(reduction="sum") on CPU in `dtype` at the values of `lprobs` [T, B, V] (targets flat).  With `logits`
    (lprobs = their log-softmax, as the criterion computes it), the gradient also flows through a log-softmax of the logits
    evaluated in `dtype`, while the CTC still sees exactly `lprobs`.
    Returns dict(nll [B] (zeroed where infinite with zero_infinity, as torch does), loss, grad = d(grad_out * loss) / d lprobs
    in torch's convention exp(lp) - posterior, grad_logits = d(grad_out * loss) / d logits or None)."""
    lp_val = lprobs.detach().cpu().to(dtype)
    x = None
    if logits is not None:
        x = logits.detach().cpu().to(dtype).requires_grad_(True)
        ls = torch.log_softmax(x, -1)
        lp = ls + (lp_val - ls).detach()   # the values of lprobs, the gradient of the log-softmax
    else:
        lp = lp_val.requires_grad_(True)
    lp.retain_grad()
    nll = F.ctc_loss(lp, targets.cpu().long(), input_lengths.cpu().long(), target_lengths.cpu().long(), blank=blank,
                     reduction="none", zero_infinity=zero_infinity)
    loss = nll.sum()
    (loss * grad_out).backward()
    return dict(nll=nll.detach(), loss=loss.detach(), grad=lp.grad, grad_logits=None if x is None else x.grad)


def prefix_initial(x, blank, dtype=np.float64):
    """State of the empty prefix (ctc_prefix_score.py:27-39): r[t] = (LOGZERO, sum_{u <= t} x[u, blank]), summed in order."""
    x = np.asarray(x, dtype=dtype)
    r = np.full((x.shape[0], 2), LOGZERO, dtype=dtype)
    r[:, 1] = np.cumsum(x[:, blank], dtype=dtype)
    return r


def prefix_score(x, last, out_len, cs, r_prev, blank, eos, dtype=np.float64):
    """One step of the prefix scorer (ctc_prefix_score.py:40-112) for nh hypotheses at once: x [T, V] log-posteriors,
    last [nh] the newest label of each prefix, out_len the labels after <sos>, cs [nh, nc] candidate labels, r_prev [nh, T, 2]
    the prefixes' states.  Returns log_psi [nh, nc] and the extensions' states r [nh, nc, T, 2]; rows before start - 1 =
    max(out_len, 1) - 1 hold LOGZERO (the reference leaves them unset: they are never read)."""
    x = np.asarray(x, dtype=dtype)
    r_prev = np.asarray(r_prev, dtype=dtype)
    cs = np.asarray(cs)
    last = np.asarray(last)
    T = x.shape[0]
    lz = np.asarray(LOGZERO, dtype=dtype)
    r = np.full((T, 2) + cs.shape, lz, dtype=dtype)
    xs = x[:, cs]                                                                   # [T, nh, nc]
    if out_len == 0:
        r[0, 0] = xs[0]
    r_sum = np.logaddexp(r_prev[:, :, 0], r_prev[:, :, 1])                        # [nh, T]
    # the label that repeats the prefix's last one may only follow a blank (:66-72)
    repeat = (out_len > 0) & (cs == last[:, None])
    log_phi = np.where(repeat[None], r_prev[:, :, 1].T[:, :, None], r_sum.T[:, :, None])
    start = max(out_len, 1)
    log_psi = r[start - 1, 0].copy()
    for t in range(start, T):
        r[t, 0] = np.logaddexp(r[t - 1, 0], log_phi[t - 1]) + xs[t]
        r[t, 1] = np.logaddexp(r[t - 1, 0], r[t - 1, 1]) + x[t, blank]
        log_psi = np.logaddexp(log_psi, log_phi[t - 1] + xs[t])
    log_psi = np.where(cs == eos, r_sum[:, -1:], log_psi)    # P(... eos | X): the prefix itself ends (:87-89)
    log_psi = np.where(cs == blank, lz, log_psi)             # (:92-94)
    return log_psi, np.transpose(r, (2, 3, 0, 1))
