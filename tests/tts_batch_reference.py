"""fp64 restatements of the batched speech-synthesis step (csrc/tts_decode.hip, T5TransformerModel.generate_speech_batch).

cross_attn: multihead_attention.py:340-389 of the reference with one query per row (softmax over the row's unpadded keys).
step_tail: the stop rule of speecht5.py:1240-1246 for B rows at one decode step, with the records the batched loop keeps.
row_limits / stop_step: the per-row length limits and the step at which a row stops, from its stop probabilities."""
import torch


def cross_attn(q, kv, k_off, S, H, hd, kpm=None):
    """q [B, >= H*hd]; kv [B*S, kv_ld] with K at column k_off and V at k_off + H*hd; kpm [B, S] (nonzero = padded key) or None.
    Returns (ctx [B, H*hd], probs [B, H, S]) in fp64."""
    B, C = q.shape[0], H * hd
    qh = q[:, :C].double().view(B, H, 1, hd) * hd ** -0.5
    k = kv[:, k_off:k_off + C].double().view(B, S, H, hd).permute(0, 2, 3, 1)     # [B, H, hd, S]
    v = kv[:, k_off + C:k_off + 2 * C].double().view(B, S, H, hd).transpose(1, 2)  # [B, H, S, hd]
    s = (qh @ k).squeeze(2)                                                        # [B, H, S]
    if kpm is not None:
        s = s.masked_fill(kpm.bool().view(B, 1, S), float("-inf"))
    p = torch.softmax(s, dim=-1)
    ctx = (p.unsqueeze(2) @ v).squeeze(2).reshape(B, C)
    return ctx, p


def step_tail(y, r, odim, minlen, maxlen, done, steps, idx, threshold, mel, probs, nxt):
    """In place on CPU tensors: y [B, >= r*odim + r]; done / steps int [B]; mel [B, cap*r, odim], probs [B, cap*r], nxt [B, odim].
    Returns the number of rows still running."""
    B = y.shape[0]
    F = r * odim
    for b in range(B):
        if int(done[b]):
            continue
        p = torch.sigmoid(y[b, F:F + r].double())
        probs[b, (idx - 1) * r:idx * r] = p.to(probs.dtype)
        mel[b, (idx - 1) * r:idx * r] = y[b, :F].view(r, odim).to(mel.dtype)
        nxt[b] = y[b, (r - 1) * odim:F].to(nxt.dtype)
        if idx >= int(minlen[b]) and (bool((p >= threshold).any()) or idx >= int(maxlen[b])):
            done[b] = 1
            steps[b] = idx
    return int((done == 0).sum())


def row_limits(T_in, r, text=True, threshold=None):
    """generate_speech's reading of its keywords (speecht5.py:1191-1201): `threshold`, when passed, is also both length ratios."""
    minr = 0.0 if threshold is None else threshold
    maxr = (20.0 if text else 10.0) if threshold is None else threshold
    thr = 0.5 if threshold is None else threshold
    minlen = [int(t * minr / r) for t in T_in]
    maxlen = [int(t * maxr / r) for t in T_in]
    return thr, minlen, maxlen, max(1, max(max(a, b) for a, b in zip(minlen, maxlen)))


def stop_step(step_probs, minlen, maxlen, threshold):
    """The 1-based step at which a row stops, given the r stop probabilities of each step (an iterable of sequences)."""
    idx = 0
    for p in step_probs:
        idx += 1
        if (any(float(v) >= threshold for v in p) or idx >= maxlen) and idx >= minlen:
            return idx
    raise AssertionError("the row did not stop within the given steps")
