"""fp64 restatement of the speaker-identification head (speaker_decoder_postnet.py of the reference) for the s2c tests: the AM / AAM
margins, F.normalize and BatchNorm1d, and the whole head from its pooled input.  Pinned to the reference fixture by
tests/test_sid_reference_cpu.py."""
import math

import torch

MARGIN_AM, MARGIN_AAM, MARGIN_AAM_EASY = 0, 1, 2


def margin(cos, target, mode, m, s, dtype=torch.float64):
    """AngularMargin / AdditiveAngularMargin forward on cosines [B, V]; target int [B] with -1 = no margin in that row.  dtype
    float32 evaluates the reference's expression in fp32 (the yardstick of the kernel tests)."""
    cos = cos.to(dtype)
    onehot = torch.zeros_like(cos)
    rows = (target >= 0).nonzero().flatten()
    onehot[rows, target[rows].long()] = 1.0
    if mode == MARGIN_AM:
        return s * (cos - m * onehot)
    sine = torch.sqrt((1.0 - cos * cos).clamp(0, 1))
    phi = cos * math.cos(m) - sine * math.sin(m)
    if mode == MARGIN_AAM_EASY:
        phi = torch.where(cos > 0, phi, cos)
    else:
        phi = torch.where(cos > math.cos(math.pi - m), phi, cos - math.sin(math.pi - m) * m)
    return s * (onehot * phi + (1.0 - onehot) * cos)


def margin_grad(cos, target, dy, mode, m, s, dtype=torch.float64):
    """d margin / d cos * dy, with the sine term's derivative taken as 0 where its clamp is active (|cos| >= 1)."""
    cos, dy = cos.to(dtype), dy.to(dtype)
    g = torch.full_like(cos, float(s))
    if mode != MARGIN_AM:
        rows = (target >= 0).nonzero().flatten()
        c = cos[rows, target[rows].long()]
        on_phi = c > 0 if mode == MARGIN_AAM_EASY else c > math.cos(math.pi - m)
        u = 1.0 - c * c
        inner = (u > 0) & (u < 1)
        dsine = torch.where(inner, math.sin(m) * c / torch.sqrt(torch.where(inner, u, torch.ones_like(u))), torch.zeros_like(u))
        g[rows, target[rows].long()] = torch.where(on_phi, s * (math.cos(m) + dsine), torch.full_like(c, float(s)))
    return g * dy


def normalize(x, eps=1e-12):
    x = x.double()
    return x / x.norm(dim=1, keepdim=True).clamp_min(eps)


def batch_norm(x, weight, bias, running_mean, running_var, training, momentum=0.1, eps=1e-5):
    """torch.nn.BatchNorm1d on [B, C] in fp64; returns (y, new_running_mean, new_running_var)."""
    x = x.double()
    if training:
        mean = x.mean(0)
        var = x.var(0, unbiased=False)
        n = x.shape[0]
        rm = (1 - momentum) * running_mean.double() + momentum * mean
        rv = (1 - momentum) * running_var.double() + momentum * var * n / (n - 1)
    else:
        mean, var = running_mean.double(), running_var.double()
        rm, rv = running_mean.double(), running_var.double()
    y = (x - mean) / torch.sqrt(var + eps) * weight.double() + bias.double()
    return y, rm, rv


def head(x, sd, args, training, target=None):
    """The SpeakerDecoderPostnet forward on pooled x [B, C] with the parameters / buffers of state dict `sd` (keys without the
    `speaker_decoder_postnet.` prefix); returns (logits, embed) in fp64."""
    x = x.double()
    if not getattr(args, "sid_no_pooling_bn", False):
        x, _, _ = batch_norm(x, sd["bn_pooling.weight"], sd["bn_pooling.bias"], sd["bn_pooling.running_mean"], sd["bn_pooling.running_var"],
                             training)
    embed = x
    if not getattr(args, "sid_no_embed_postnet", False):
        e = x @ sd["output_embedding.weight"].double().t()
        embed, _, _ = batch_norm(e, sd["bn_embedding.weight"], sd["bn_embedding.bias"], sd["bn_embedding.running_mean"],
                                 sd["bn_embedding.running_var"], training)
    kind = getattr(args, "sid_softmax_type", "softmax")
    W = sd["output_projection.weight"].double()
    if kind != "softmax" or getattr(args, "sid_normalize_postnet", False):
        out = normalize(embed) @ normalize(W).t()
        if training and target is not None and kind != "softmax":
            mode = MARGIN_AM if kind == "amsoftmax" else (MARGIN_AAM_EASY if args.softmax_easy_margin else MARGIN_AAM)
            out = margin(out, target, mode, args.softmax_margin, args.softmax_scale)
        return out, embed
    return embed @ W.t(), embed
