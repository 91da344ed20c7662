"""The contract of st5_ctc_pack_rows (include/speecht5_hip.h) restated in numpy, element by element -- no masked_select, no cumsum:
the GPU tests compare the kernel with this, tests/test_ctc_pack_cpu.py compares this with torch's masked_select + cumsum form."""
import numpy as np


def pack_rows(target, pad, eos):
    """target int64 [B, L] -> (packed [B, L], offsets [B], kept [B], total [1]), all int64.  Row b of `packed`: the entries of
    target[b] that are neither pad nor eos, in order, from column 0; the rest pad.  offsets[b] = b * L."""
    target = np.asarray(target, dtype=np.int64)
    B, L = target.shape
    packed = np.full((B, L), pad, dtype=np.int64)
    kept = np.zeros(B, dtype=np.int64)
    for b in range(B):
        k = 0
        for i in range(L):
            v = int(target[b, i])
            if v != pad and v != eos:
                packed[b, k] = v
                k += 1
        kept[b] = k
    offsets = np.arange(B, dtype=np.int64) * L
    return packed, offsets, kept, np.array([int(kept.sum())], dtype=np.int64)


def rows_of_every_kind(B, L, pad, eos, vocab, seed):
    """int64 [B, L] with, in turn: an all-pad row, an eos-only row, a full row without pad or eos, label + eos + pad (the collater's
    row), an eos in mid-row, a random mixture -- row b is of kind (b + L) % 6, so that a set of shapes with few rows still meets every
    kind.  Labels lie in [4, vocab)."""
    rng = np.random.RandomState(seed)
    t = rng.randint(4, vocab, size=(B, L)).astype(np.int64)
    for b in range(B):
        kind = (b + L) % 6
        if kind == 0:
            t[b] = pad
        elif kind == 1:
            t[b] = pad
            t[b, 0] = eos
        elif kind == 3:
            n = int(rng.randint(0, L))
            t[b, n] = eos
            t[b, n + 1:] = pad
        elif kind == 4:
            t[b, L // 2] = eos
        elif kind == 5:
            m = rng.randint(0, 4, size=L)
            t[b, m == 0] = pad
            t[b, m == 1] = eos
    return t
