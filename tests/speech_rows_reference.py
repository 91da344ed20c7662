"""fp64 torch restatement of the speech encoder pre-net in two forms, for the length-exact batched encoding
(T5TransformerModel.forward_encoder_rows):

  prenet(sd, cfg, wav, padding_mask)            the reference's padded batch (SpeechEncoderPrenet._forward without span mask): conv
                                                layer 0's GroupNorm over all frames of the padded row, the chunk padding mask, the
                                                positional convolution over whatever the padded frames hold;
  prenet(sd, cfg, wav, lens=[n_b])              the length-aware form: GroupNorm over the row's own L0_b frames, zeros behind them,
                                                the mask t >= T_b from the conv length formula, frames t >= T_b zero when the
                                                positional convolution runs.

A single clip is prenet(sd, cfg, wav[b:b+1, :n_b], all-False mask): tests/test_speech_rows_cpu.py pins that form to the verbatim
oracle (oracle.speecht5_oracle.speech_encoder_prenet) and shows that the aware batch equals the single clips while the unaware batch
does not.  Everything runs in the dtype of `sd` / `wav` (fp64 in the tests); the sinusoidal table and the position rule are the
oracle's own functions."""
import torch
import torch.nn.functional as F

from oracle.speecht5_oracle import fairseq_positions, fairseq_sinusoidal_table

LENGTHS = [16000, 40000, 27200, 400, 16079, 16080]      # samples; 400 = one frame, 16079 / 16080 straddle a frame boundary
PRE = "speech_encoder_prenet."


def layers_of(cfg):
    return eval(cfg.conv_feature_layers)  # noqa


def frames(n, layers):
    for _, k, s in layers:
        n = (n - k) // s + 1
    return n


def padded_batch(lengths, seed=0, dtype=torch.float64, fill=0.0):
    """Right-padded waveforms [B, max n] (padding = `fill`), the bool padding mask, and the unpadded clips."""
    g = torch.Generator().manual_seed(seed)
    S = max(lengths)
    wav = torch.full((len(lengths), S), fill, dtype=dtype)
    pad = torch.ones(len(lengths), S, dtype=torch.bool)
    clips = []
    for b, n in enumerate(lengths):
        c = (torch.randn(n, generator=g, dtype=torch.float64) * 0.1).to(dtype)
        wav[b, :n] = c
        pad[b, :n] = False
        clips.append(c)
    return wav, pad, clips


def extractor(sd, cfg, wav, lens=None):
    """ConvFeatureExtractionModel.forward, channels-last out [B, T, C]; `lens` (samples per row) selects the length-aware layer 0."""
    layers = layers_of(cfg)
    p0 = PRE + "feature_extractor."
    x = wav.unsqueeze(1)
    for i, (dim, k, s) in enumerate(layers):
        p = f"{p0}conv_layers.{i}."
        x = F.conv1d(x, sd[p + "0.weight"], sd.get(p + "0.bias"), stride=s)
        if cfg.extractor_mode == "layer_norm":
            x = F.layer_norm(x.transpose(-2, -1), (dim,), sd[p + "2.1.weight"], sd[p + "2.1.bias"]).transpose(-2, -1)
            x = F.gelu(x)
        elif i == 0:
            if lens is None:
                x = F.gelu(F.group_norm(x, dim, sd[p + "2.weight"], sd[p + "2.bias"], 1e-5))
            else:
                y = torch.zeros_like(x)
                for b, n in enumerate(lens):
                    L0 = (n - k) // s + 1
                    y[b:b + 1, :, :L0] = F.gelu(F.group_norm(x[b:b + 1, :, :L0], dim, sd[p + "2.weight"], sd[p + "2.bias"], 1e-5))
                x = y
        else:
            x = F.gelu(x)
    return x.transpose(1, 2)


def chunk_mask(padding_mask, T):
    """SpeechEncoderPrenet.forward_padding_mask: frame t is padded when all of its chunk of samples is."""
    extra = padding_mask.size(1) % T
    pm = padding_mask[:, :-extra] if extra > 0 else padding_mask
    return pm.view(pm.size(0), T, -1).all(-1)


def exact_mask(lens, T, layers):
    return torch.arange(T)[None, :] >= torch.tensor([frames(n, layers) for n in lens])[:, None]


def prenet(sd, cfg, wav, padding_mask=None, lens=None):
    """-> (x [B, T, d], frame padding mask [B, T]).  Exactly one of `padding_mask` (reference form) / `lens` (aware form)."""
    assert (padding_mask is None) != (lens is None)
    x = extractor(sd, cfg, wav, lens)
    T = x.size(1)
    x = F.layer_norm(x, (x.shape[-1],), sd[PRE + "layer_norm.weight"], sd[PRE + "layer_norm.bias"], 1e-5)
    pm = chunk_mask(padding_mask, T) if lens is None else exact_mask(lens, T, layers_of(cfg))
    if (PRE + "post_extract_proj.weight") in sd:
        x = F.linear(x, sd[PRE + "post_extract_proj.weight"], sd[PRE + "post_extract_proj.bias"])
    if lens is not None:
        x = x.masked_fill(pm[:, :, None], 0.0)
    if cfg.use_conv_pos:
        v, g = sd[PRE + "pos_conv.0.weight_v"], sd[PRE + "pos_conv.0.weight_g"]
        w = v * (g / v.norm(dim=(0, 1), keepdim=True))
        k = cfg.conv_pos
        pos = F.conv1d(x.transpose(1, 2), w, sd[PRE + "pos_conv.0.bias"], padding=k // 2, groups=cfg.conv_pos_groups)
        if k % 2 == 0:
            pos = pos[:, :, :-1]
        x = x + F.gelu(pos).transpose(1, 2)
    if cfg.use_sinc_pos:
        positions = fairseq_positions(~pm, 1)
        table = fairseq_sinusoidal_table(int(positions.max()) + 2, x.shape[-1], 1).to(x.dtype)
        x = x + table[positions]
    return x, pm


def single(sd, cfg, clip):
    """One unpadded clip [n] through the reference form."""
    return prenet(sd, cfg, clip[None, :], padding_mask=torch.zeros(1, clip.numel(), dtype=torch.bool))


def rel_err(a, b):
    """max-norm error of a against b, relative to b's largest magnitude."""
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
