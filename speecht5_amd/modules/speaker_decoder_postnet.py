"""SpeakerDecoderPostnet mirror of SpeechT5/speecht5/models/modules/speaker_decoder_postnet.py:130-197 (speaker identification,
t5_task s2c): same parameter / buffer names and init, so `speecht5_sid.pt`-style checkpoints load key for key.

    x [B, C] -> [bn_pooling] -> [output_embedding -> bn_embedding] = embed -> output_projection(embed)            (softmax head)
                                                                          -> cos(embed, W) [-> AM / AAM margin]    (normalised head)

The head runs in fp32 (B rows): BatchNorm1d on st5_batchnorm_act_*, the projections on st5_gemm, F.normalize on st5_norm_rows and the
margin on st5_angular_margin_* (functional.row_batch_norm / linear / cosine_logits).  As in the reference, the margin is applied only
in training and only when a target is given.  Logits are fp32 [B, class_num] views whose row stride is padded (class_num is odd)."""
import math

import torch
import torch.nn as nn

from .. import functional as Fn


class AngularMargin(nn.Module):
    """Constants of the reference's AngularMargin (AM); applied by st5_angular_margin_fwd."""

    def __init__(self, margin=0.0, scale=1.0):
        super().__init__()
        self.margin = margin
        self.scale = scale

    def kernel_cfg(self):
        return (Fn.MARGIN_AM, self.margin, self.scale)


class AdditiveAngularMargin(AngularMargin):
    """Constants of the reference's AdditiveAngularMargin (AAM); applied by st5_angular_margin_fwd."""

    def __init__(self, margin=0.0, scale=1.0, easy_margin=False):
        super().__init__(margin, scale)
        self.easy_margin = easy_margin
        self.cos_m = math.cos(self.margin)
        self.sin_m = math.sin(self.margin)
        self.th = math.cos(math.pi - self.margin)
        self.mm = math.sin(math.pi - self.margin) * self.margin

    def kernel_cfg(self):
        return (Fn.MARGIN_AAM_EASY if self.easy_margin else Fn.MARGIN_AAM, self.margin, self.scale)


class SpeakerDecoderPostnet(nn.Module):
    def __init__(self, embed_dim, class_num, args):
        super().__init__()
        self.embed_dim = embed_dim
        self.class_num = class_num
        self.no_pooling_bn = getattr(args, "sid_no_pooling_bn", False)
        self.no_embed_postnet = getattr(args, "sid_no_embed_postnet", False)
        self.normalize_postnet = getattr(args, "sid_normalize_postnet", False)
        self.softmax_head = getattr(args, "sid_softmax_type", "softmax")
        if not self.no_pooling_bn:
            self.bn_pooling = nn.BatchNorm1d(args.decoder_output_dim)
        else:
            self.bn_pooling = None
        if not self.no_embed_postnet:
            self.output_embedding = nn.Linear(args.decoder_output_dim, embed_dim, bias=False)
            self.bn_embedding = nn.BatchNorm1d(embed_dim)
        else:
            self.output_embedding = None
            self.bn_embedding = None
            self.embed_dim = args.decoder_output_dim
        self.output_projection = nn.Linear(self.embed_dim, class_num, bias=False)
        if self.softmax_head == "amsoftmax":
            self.output_layer = AngularMargin(args.softmax_margin, args.softmax_scale)
        elif self.softmax_head == "aamsoftmax":
            self.output_layer = AdditiveAngularMargin(args.softmax_margin, args.softmax_scale, args.softmax_easy_margin)
        else:
            self.output_layer = None
        if self.output_embedding is not None:
            nn.init.normal_(self.output_embedding.weight, mean=0, std=embed_dim ** -0.5)
        nn.init.normal_(self.output_projection.weight, mean=0, std=class_num ** -0.5)

    def forward(self, x, target=None):
        """x [B, C] (any float dtype); target: int64 class per row [B] (-1 = none) or None.  Returns (logits fp32 [B, class_num],
        embed fp32 [B, embed_dim]).  The reference takes a one-hot [B, class_num] target; T5TransformerModel passes its argmax."""
        x = Fn.as_float(x)
        if self.bn_pooling is not None:
            x = Fn.row_batch_norm(x, self.bn_pooling)
        if self.output_embedding is not None and self.bn_embedding is not None:
            embed = Fn.row_batch_norm(Fn.linear(x.contiguous(), self.output_embedding.weight), self.bn_embedding)
        else:
            embed = x
        if self.output_layer is not None or self.normalize_postnet:
            margin = None
            if self.training and target is not None and self.output_layer is not None:
                margin = self.output_layer.kernel_cfg()
            output = Fn.cosine_logits(embed, self.output_projection.weight, target if margin is not None else None, margin)
        else:
            output = Fn.linear(embed.contiguous(), self.output_projection.weight)
        return output, embed
