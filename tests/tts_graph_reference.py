"""Restatements for the device-stepped / graph-replayed TTS decode (speecht5_amd/tts_graph.py, csrc/decode_gemm.hip):
the eager decode loop's control flow as plain Python, and the skinny-M GEMM with its epilogues in fp64."""
import math

import torch

ACT_NONE, ACT_GELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3

# (N, K) the kernel serves: the Base decode step, the tiny golden model's step, the shallow-fusion LM's layers
BASE_SHAPES = [(256, 80), (256, 256), (768, 256), (768, 1280), (768, 768), (1536, 768), (2304, 768), (3072, 768), (768, 3072), (162, 768)]
TINY_SHAPES = [(32, 80), (32, 32), (128, 32), (128, 192), (128, 128), (256, 128), (384, 128), (128, 256), (162, 128)]
LM_SHAPES = [(1280, 1280), (2560, 1280), (3840, 1280), (6144, 1280), (1280, 6144)]


def eager_loop(cap, poll_steps, stop_at_poll=None):
    """(steps run, polls taken) of T5TransformerModel._decode_rows' loop: a poll behind step idx when idx % poll_steps == 0 and
    idx < cap; the loop ends at the poll numbered `stop_at_poll` (1-based), which reports no active row."""
    steps, polls = [], []
    for idx in range(1, cap + 1):
        steps.append(idx)
        if idx % poll_steps == 0 and idx < cap:
            polls.append(idx)
            if stop_at_poll is not None and len(polls) == stop_at_poll:
                break
    return steps, polls


def act64(x, act):
    if act == ACT_GELU:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == ACT_RELU:
        return x.clamp_min(0.0)
    if act == ACT_TANH:
        return torch.tanh(x)
    return x


def skinny_gemm(x, weights, biases=None, act=ACT_NONE, residual=None):
    """fp64: act(x . stack(weights)^T + stack(biases)) + residual, the epilogue order of st5_gemm_skinny at dropout 0."""
    w = torch.cat([w_.double() for w_ in weights], dim=0)
    y = x.double() @ w.t()
    if biases is not None:
        y = y + torch.cat([b.double() for b in biases], dim=0)
    y = act64(y, act)
    if residual is not None:
        y = y + residual.double()
    return y


def ulp_at_scale(ref, dtype):
    """One unit in the last place of `dtype` at the magnitude of the largest reference value."""
    s = float(ref.abs().max())
    if s == 0.0:
        return 0.0
    bits = 23 if dtype == torch.float32 else 7
    return 2.0 ** (math.floor(math.log2(s)) - bits)
