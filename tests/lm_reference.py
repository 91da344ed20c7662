"""fp64 / fp32 restatement of fairseq's `transformer_lm` as `transformer_lm_t5` configures it (speecht5_amd/transformer_lm.py is
the HIP model): sqrt(d)-scaled token embedding + fairseq sinusoidal positions (pad tokens at position `pad`), pre-LN layers
with causal self-attention and a key-padding mask, exact-erf GELU FFN, final LayerNorm, output projection without bias.
Torch on the host in the dtype of the given state dict; tests/test_lm_reference_cpu.py pins it to the fixture the verbatim
reference layers wrote (tests/golden/tiny_s2t_beam_lm.pt)."""
import math

import torch
import torch.nn.functional as F


def sinusoidal(n, dim, pad, dtype=torch.float64):
    """fairseq SinusoidalPositionalEmbedding.get_embedding (computed in fp32 as fairseq does, then cast)."""
    half = dim // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float) * -(math.log(10000) / (half - 1)))
    ang = torch.arange(n, dtype=torch.float).unsqueeze(1) * freq.unsqueeze(0)
    emb = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    emb[pad] = 0
    return emb.to(dtype)


def positions(tokens, pad):
    m = tokens.ne(pad).long()
    return torch.cumsum(m, dim=1) * m + pad


def _ln(x, sd, key):
    return F.layer_norm(x, (x.shape[-1],), sd[key + ".weight"], sd[key + ".bias"], 1e-5)


def _lin(x, sd, key, bias=True):
    return F.linear(x, sd[key + ".weight"], sd.get(key + ".bias") if bias else None)


def lm_forward(sd, tokens, heads, pad=1, act="gelu"):
    """sd: fairseq-layout state dict (any float dtype; the computation runs in that dtype).  tokens [B, T].
    Returns (logits [B, T, V], inner states [B, T, C] * (L + 1): the embedding output and every layer's output)."""
    emb = sd["decoder.embed_tokens.weight"]
    dt = emb.dtype
    tokens = tokens.to(emb.device)
    B, T = tokens.shape
    C = emb.shape[1]
    hd = C // heads
    pos = positions(tokens, pad)
    x = math.sqrt(C) * emb[tokens] + sinusoidal(pad + T + 1, C, pad, dt).to(emb.device)[pos]
    padm = tokens.eq(pad)
    causal = torch.triu(torch.ones(T, T, dtype=torch.bool, device=tokens.device), 1)
    mask = causal.view(1, 1, T, T) | padm.view(B, 1, 1, T)
    fn = {"gelu": F.gelu, "relu": F.relu, "tanh": torch.tanh, "linear": lambda v: v}[act]
    states = [x]
    n = 0
    while f"decoder.layers.{n}.fc1.weight" in sd:
        p = f"decoder.layers.{n}."
        h = _ln(x, sd, p + "self_attn_layer_norm")
        q = _lin(h, sd, p + "self_attn.q_proj").view(B, T, heads, hd).transpose(1, 2) * hd ** -0.5
        k = _lin(h, sd, p + "self_attn.k_proj").view(B, T, heads, hd).transpose(1, 2)
        v = _lin(h, sd, p + "self_attn.v_proj").view(B, T, heads, hd).transpose(1, 2)
        s = (q @ k.transpose(-1, -2)).masked_fill(mask, float("-inf"))
        a = torch.softmax(s, dim=-1) @ v
        x = x + _lin(a.transpose(1, 2).reshape(B, T, C), sd, p + "self_attn.out_proj")
        h = _ln(x, sd, p + "final_layer_norm")
        x = x + _lin(fn(_lin(h, sd, p + "fc1")), sd, p + "fc2")
        states.append(x)
        n += 1
    x = _ln(x, sd, "decoder.layer_norm")
    w = sd.get("decoder.output_projection.weight", emb)
    return F.linear(x, w), states


def lm_log_probs(logits):
    return torch.log_softmax(logits, dim=-1)
