"""The definition of the state digest (csrc/state_digest_index.h, st5_state_digest, checkpoint.host_digest), restated in numpy on
vectorised uint64 -- what the kernel, the host program built from the header and checkpoint.py's host digest are compared against.

All arithmetic mod 2^64, for a segment of n bytes:
    w_i     the little-endian 8-byte words of the segment, the last one zero-padded
    digest  = h((sum over i of h(w_i + (i + 1) * 0x9E3779B97F4A7C15)) + n)
    h       the splitmix64 finaliser"""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15


def splitmix64_finaliser(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def digest(data):
    """data: bytes, or anything numpy turns into an array; its bytes in memory order are the segment.  Returns a Python int."""
    raw = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    n = raw.size
    padded = np.zeros((n + 7) // 8 * 8, dtype=np.uint8)
    padded[:n] = raw
    words = padded.view("<u8").astype(np.uint64)
    with np.errstate(over="ignore"):
        position = np.arange(1, words.size + 1, dtype=np.uint64) * np.uint64(GOLDEN)
        total = splitmix64_finaliser(words + position).sum(dtype=np.uint64) if words.size else np.uint64(0)
        return int(splitmix64_finaliser(np.array([total], dtype=np.uint64) + np.uint64(n))[0])


SIZES = [0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 4097]
OFFSETS = [0, 1, 4, 8]


def pattern(n, seed):
    """n reproducible bytes (a 64-bit LCG, its high byte): the same in the host program of tests/test_checkpoint_cpu.py."""
    out = np.empty(n, dtype=np.uint8)
    x = (seed * 2862933555777941757 + 3037000493) & 0xFFFFFFFFFFFFFFFF
    for i in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out[i] = x >> 56
    return out
