"""T5TransformerModel mirror of SpeechT5/speecht5/models/speecht5.py:47-1447: same registration names
(`t5_transformer` + archs), constructor/builders, forward routing, inference entry points and state-dict
keys, with every module running on the gfx950 HIP kernels (speecht5_amd/csrc)."""
import contextlib
import logging
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import functional as Fn
from .fairseq_compat import FairseqEncoderDecoderModel, register_model, register_model_architecture
from .modules import (GumbelVectorQuantizer, SpeechDecoderPostnet, SpeechDecoderPrenet, SpeechEncoderPostnet,
                      SpeechEncoderPrenet, TextDecoderPostnet, TextDecoderPrenet, TextEncoderPrenet, TransformerDecoder,
                      TransformerEncoder)
from .modules.speaker_decoder_postnet import SpeakerDecoderPostnet

logger = logging.getLogger(__name__)

DEFAULT_MAX_TEXT_POSITIONS = 450
DEFAULT_MAX_SPEECH_POSITIONS = 4000


def Embedding(num_embeddings, embedding_dim, padding_idx):
    m = nn.Embedding(num_embeddings, embedding_dim, padding_idx=padding_idx)
    nn.init.normal_(m.weight, mean=0, std=embedding_dim ** -0.5)
    nn.init.constant_(m.weight[padding_idx], 0)
    return m


def init_bert_params(module):
    """fairseq init_bert_params: N(0, 0.02) for Linear / Embedding / MHA q,k,v weights; zero biases and pad row."""
    from .modules import MultiheadAttention

    def normal_(data):
        data.copy_(data.cpu().normal_(mean=0.0, std=0.02).to(data.device))

    if isinstance(module, nn.Linear):
        normal_(module.weight.data)
        if module.bias is not None:
            module.bias.data.zero_()
    if isinstance(module, nn.Embedding):
        normal_(module.weight.data)
        if module.padding_idx is not None:
            module.weight.data[module.padding_idx].zero_()
    if isinstance(module, MultiheadAttention):
        normal_(module.q_proj.weight.data)
        normal_(module.k_proj.weight.data)
        normal_(module.v_proj.weight.data)


def tts_row_limits(T_in, reduction_factor, text, **kwargs):
    """Stop threshold, per-row minlen_b / maxlen_b and the step cap of generate_speech_batch for encoder lengths T_in, with the
    keywords read exactly as generate_speech reads them: `threshold` also stands for both length ratios when it is passed
    (speecht5.py:1191-1201); otherwise 0.5, 0.0 and 20.0 (text) / 10.0 (speech)."""
    threshold = kwargs.get("threshold", 0.5)
    minlenratio = kwargs.get("threshold", 0.0)
    maxlenratio = kwargs.get("threshold", 20.0 if text else 10.0)
    minlen = [int(t * minlenratio / reduction_factor) for t in T_in]
    maxlen = [int(t * maxlenratio / reduction_factor) for t in T_in]
    cap = max(1, max(max(a, b) for a, b in zip(minlen, maxlen)))
    return threshold, minlen, maxlen, cap


@register_model("t5_transformer")
class T5TransformerModel(FairseqEncoderDecoderModel):
    def __init__(self, args, encoder, decoder, text_encoder_prenet, speech_encoder_prenet, text_decoder_prenet,
                 speech_decoder_prenet, text_decoder_postnet, speech_decoder_postnet, speaker_decoder_postnet,
                 speech_encoder_postnet):
        super().__init__(encoder, decoder)
        self.encoder = encoder
        self.decoder = decoder
        self.text_encoder_prenet = text_encoder_prenet
        self.speech_encoder_prenet = speech_encoder_prenet
        self.text_decoder_prenet = text_decoder_prenet
        self.speech_decoder_prenet = speech_decoder_prenet
        self.text_decoder_postnet = text_decoder_postnet
        self.speech_decoder_postnet = speech_decoder_postnet
        self.speaker_decoder_postnet = speaker_decoder_postnet
        self.hubert_layer = speech_encoder_postnet
        self.reduction_factor = args.reduction_factor
        self.spk_embed_dim = args.spk_embed_dim
        self.spk_embed_integration_type = args.spk_embed_integration_type
        if self.spk_embed_dim is not None and self.spk_embed_integration_type != "pre":
            raise NotImplementedError("speaker-embedding integration other than 'pre' is not used by the recipes")
        self.use_codebook = args.use_codebook
        self.codebook_prob = getattr(args, "codebook_prob", 0.5)
        if self.use_codebook:
            vq_dim = args.latent_dim if args.latent_dim > 0 else args.encoder_embed_dim
            self.quantizer = GumbelVectorQuantizer(dim=args.encoder_embed_dim, num_vars=args.latent_vars, temp=args.latent_temp,
                                                   groups=args.latent_groups, combine_groups=False, vq_dim=vq_dim, time_first=True,
                                                   weight_proj_depth=args.quantizer_depth, weight_proj_factor=args.quantizer_factor)
        self.num_updates = 0
        if args.bert_init:
            self.apply(init_bert_params)
        self.args = args

    @staticmethod
    def add_args(parser):
        """Model options, speecht5.py:117-614 of the reference (same names / dests / defaults: speecht5_amd/cli.py)."""
        from . import cli
        cli.declare(parser, cli.MODEL_OPTIONS)

    # ---- builders (speecht5.py:616-729) ----
    @classmethod
    def build_encoder(cls, args, dictionary=None, embed_tokens=None):
        return TransformerEncoder(args, dictionary, embed_tokens)

    @classmethod
    def build_decoder(cls, args):
        return TransformerDecoder(args)

    @classmethod
    def build_text_encoder_prenet(cls, embed_tokens, args):
        return TextEncoderPrenet(embed_tokens, args)

    @classmethod
    def build_speech_encoder_prenet(cls, args):
        return SpeechEncoderPrenet(args)

    @classmethod
    def build_text_decoder_prenet(cls, embed_tokens, args):
        return TextDecoderPrenet(embed_tokens, args)

    @classmethod
    def build_speech_decoder_prenet(cls, odim, args):
        return SpeechDecoderPrenet(odim, args)

    @classmethod
    def build_text_decoder_postnet(cls, embed_tokens, dictionary, args):
        return TextDecoderPostnet(embed_tokens, dictionary, args)

    @classmethod
    def build_speech_decoder_postnet(cls, odim, args):
        return SpeechDecoderPostnet(odim, args)

    @classmethod
    def build_speech_encoder_postnet(cls, dictionaries, args):
        return SpeechEncoderPostnet(dictionaries, args)

    @classmethod
    def build_speaker_decoder_postnet(cls, embed_dim, class_num, args):
        return SpeakerDecoderPostnet(embed_dim, class_num, args)

    @staticmethod
    def check_s2c_options(args):
        """The speaker-identification options this project does not implement are refused by name (speecht5.py:674-713,
        :818-842, :912-932 of the reference); the recipe uses none of them."""
        pooling = getattr(args, "sid_pooling_layer", "decoder")
        if pooling in ("decoder-las", "encoder-speaker"):
            raise NotImplementedError(f"--sid-pooling-layer {pooling} is not implemented (decoder, encoder and encoder-cls are)")
        for flag in ("sid_decoder_speaker", "sid_t5_postnet", "sid_shuffle_encoder_input", "sid_pad_prenet"):
            if getattr(args, flag, False):
                raise NotImplementedError(f"--{flag.replace('_', '-')} is not implemented for s2c")
        if getattr(args, "sid_encoder_cls", None) is not None:
            raise NotImplementedError("--sid-encoder-cls is not implemented for s2c")
        if pooling not in ("decoder", "encoder", "encoder-cls"):
            raise ValueError(f"unknown --sid-pooling-layer {pooling!r}")

    @classmethod
    def build_model(cls, args, task):
        base_architecture(args)

        def build_embedding(dictionary, embed_dim):
            return Embedding(len(dictionary), embed_dim, dictionary.pad())

        text_decoder_embed_tokens = build_embedding(task.dicts["text"], args.decoder_embed_dim)
        if args.share_input_output_embed:
            text_encoder_embed_tokens = text_decoder_embed_tokens
        else:
            text_encoder_embed_tokens = build_embedding(task.dicts["text"], args.encoder_embed_dim)
        speech_odim = args.speech_odim
        if "text" in task.dicts:
            encoder = cls.build_encoder(args, task.dicts["text"], text_encoder_embed_tokens)
        else:
            encoder = cls.build_encoder(args)
        decoder = cls.build_decoder(args)
        text_encoder_prenet = cls.build_text_encoder_prenet(text_encoder_embed_tokens, args)
        speech_encoder_prenet = cls.build_speech_encoder_prenet(args)
        text_decoder_prenet = cls.build_text_decoder_prenet(text_decoder_embed_tokens, args)
        speech_decoder_prenet = cls.build_speech_decoder_prenet(speech_odim, args)
        text_decoder_postnet = cls.build_text_decoder_postnet(text_decoder_embed_tokens, task.dicts["text"], args)
        speech_decoder_postnet = cls.build_speech_decoder_postnet(speech_odim, args)
        speaker_decoder_postnet = None
        if getattr(task, "t5_task", None) == "s2c":
            cls.check_s2c_options(args)
            speaker_decoder_postnet = cls.build_speaker_decoder_postnet(args.sid_embed_dim, len(task.dicts["text"]), args)
        speech_encoder_postnet = cls.build_speech_encoder_postnet(task.dicts["hubert"], args) if "hubert" in task.dicts else None
        return cls(args, encoder, decoder, text_encoder_prenet, speech_encoder_prenet, text_decoder_prenet,
                   speech_decoder_prenet, text_decoder_postnet, speech_decoder_postnet, speaker_decoder_postnet, speech_encoder_postnet)

    # ---- criterion-facing helpers (speecht5.py:731-784) ----
    def get_normalized_probs(self, net_output, log_probs, sample=None):
        logits = net_output[0]
        lprobs = F.log_softmax(logits.float(), dim=-1) if log_probs else F.softmax(logits.float(), dim=-1)
        lprobs.batch_first = True
        return lprobs

    def get_normalized_probs_for_ctc(self, net_output, log_probs):
        logits = net_output["encoder_out_for_ctc"][0]
        return F.log_softmax(logits.float(), dim=-1) if log_probs else F.softmax(logits.float(), dim=-1)

    def get_logits(self, net_output, is_masked=True):
        logits_list = net_output["logit_m_list"] if is_masked else net_output["logit_u_list"]
        return [x.float() for x in logits_list if x is not None]

    def get_targets(self, sample, net_output, is_masked=True):
        if "logit_m_list" in net_output:
            sel = net_output.get("sel_m" if is_masked else "sel_u")
            if sel is not None:
                # fixed-shape form (recorded / replayed steps): logits of ALL frames; the frames outside the (un)masked set
                # get the ignored target -1, the others class 0 as in the reference
                return [(sel.long() - 1) for _ in self.get_logits(net_output, is_masked)]
            return [x.new_zeros(x.size(0), dtype=torch.long) for x in self.get_logits(net_output, is_masked)]
        return sample["target"]

    def get_target_count(self, net_output, is_masked=True):
        """Number of frames the (un)masked prediction loss runs over: the reference's `targ_list[0].numel()`
        (speech_pretrain_criterion.py:117,127) -- a Python int, or a device scalar in the fixed-shape form."""
        sel = net_output.get("sel_m" if is_masked else "sel_u")
        if sel is not None:
            return sel.sum().float()
        lg = self.get_logits(net_output, is_masked)
        return lg[0].size(0) if lg else 0

    def get_extra_losses(self, net_output):
        extra_losses, names = [], []
        if "features_pen" in net_output:
            extra_losses.append(net_output["features_pen"])
            names.append("features_pen")
        if "prob_perplexity" in net_output:
            extra_losses.append((net_output["num_vars"] - net_output["prob_perplexity"]) / net_output["num_vars"])
            names.append("prob_perplexity")
        return extra_losses, names

    def max_positions(self):
        return None

    def max_decoder_positions(self):
        return self.args.max_text_positions

    # ---- forward (speecht5.py:786-963) ----
    def forward(self, source=None, src_tokens=None, src_lengths=None, prev_output_tokens=None, tgt_lengths=None, spkembs=None,
                target_list=None, task_name=None, padding_mask=None, only_hubert=False, only_ctc=False, feature_only=False,
                tgt_enc_layer=None, mask=True, tgt_live=None):
        """tgt_live (not in the reference): int32 [1] on the device, the decoder steps of the batch the own-length collater would have
        built (collate.TextToSpeechCollater(fixed_shape=...) sets it: max length // reduction factor).  t2s only: the mel post-net's
        convolutions and batch statistics then range over those steps' frames alone."""
        assert source is not None or src_tokens is not None
        if tgt_live is not None and task_name != "t2s":
            raise ValueError(f"tgt_live is the t2s route's (task_name {task_name!r}): only the text-to-speech fixed-shape batch has it")
        input_type = "text" if (source is None and padding_mask is None and not feature_only) else "speech"
        if prev_output_tokens is not None and len(prev_output_tokens.size()) == 2:
            output_type = "text"
            codebook_out = {}
        else:
            output_type = "speech"
        sid_target = None
        if task_name is not None and task_name == "s2c":
            # (:805-810) the reference's one-hot sid_target, kept as the class index; the collater never passes target_list, so in
            # the recipe the margin is never applied
            if target_list is not None and target_list.size(1) == 1:
                sid_target = target_list.squeeze(1)
            target_list = None

        # Encoder pre-net
        if input_type == "text":
            encoder_input, encoder_padding_mask = self.text_encoder_prenet(src_tokens)
        elif target_list is not None:
            encoder_input, encoder_padding_mask = self.speech_encoder_prenet(
                source, require_feat_pen=True, target_list=target_list, padding_mask=padding_mask, mask=mask)
            encoder_input, features_pen, mask_indices, target_list = encoder_input
        else:
            encoder_input, encoder_padding_mask = self.speech_encoder_prenet(source, padding_mask=padding_mask, mask=self.training)

        encoder_output = self.encoder(encoder_input, encoder_padding_mask, tgt_layer=tgt_enc_layer)

        if task_name is not None and task_name == "speech_pretrain" and feature_only:
            return encoder_output["encoder_out"][0].transpose(0, 1)

        if task_name is not None and task_name == "s2c":   # (:836-842) encoder pooling, before the codebook mix
            pooling = self.args.sid_pooling_layer
            if pooling == "encoder":   # mean over ALL frames, padded ones included
                return self.speaker_decoder_postnet(Fn.time_mean(encoder_output["encoder_out"][0]), sid_target), None
            if pooling == "encoder-cls":
                return self.speaker_decoder_postnet(encoder_output["encoder_out"][0][0], sid_target), None

        if target_list is not None:
            hubert_results = self.hubert_layer(encoder_output["encoder_out"][0].transpose(0, 1), encoder_padding_mask,
                                               mask_indices, target_list)
            hubert_results["features_pen"] = features_pen

        if "decoder_input" in encoder_output and encoder_output["decoder_input"][0] is not None:
            encoder_output["encoder_out"] = encoder_output["decoder_input"]

        if self.use_codebook:
            enc_btc = encoder_output["encoder_out"][0].transpose(0, 1)
            tlen = enc_btc.size(1)
            n_mix = int(tlen * self.codebook_prob)

            def draw_mix():   # built on the host: no device-side index_put / sync
                w = torch.zeros(tlen)
                w[torch.randperm(tlen)[:n_mix]] = 1.0
                return w
            q_w = Fn.stage_host(draw_mix, enc_btc.device)
            # quantised codes, mixed time-wise with the encoder states (:870-877) inside the quantizer's kernel
            q = self.quantizer(enc_btc.contiguous(), mix_w=q_w)
            encoder_output["encoder_out"][0] = q["x"].transpose(0, 1)
            tgt = hubert_results if output_type == "speech" else codebook_out
            tgt["prob_perplexity"] = q["prob_perplexity"]
            tgt["code_perplexity"] = q["code_perplexity"]
            tgt["num_vars"] = q["num_vars"]
            tgt["temp"] = q["temp"]

        if only_hubert and target_list is not None:
            return hubert_results, None
        if only_ctc and task_name is not None and task_name == "s2t":
            return None, encoder_output
        elif not self.training and prev_output_tokens is None and task_name == "s2t" and task_name is not None:
            return encoder_output

        # Decoder pre-net
        if task_name is not None and task_name == "s2c":
            # (:893-896) the pre-net's output is replaced by zeros: nothing of it (nor a gradient) reaches the decoder
            prev_output_tokens, tgt_mask = self._zero_decoder_input(prev_output_tokens)
        elif output_type == "text":
            prev_output_tokens, tgt_mask, _ = self.text_decoder_prenet(prev_output_tokens)
        else:
            prev_output_tokens, tgt_mask = self.speech_decoder_prenet(prev_output_tokens, tgt_lengths, spkembs)
        if task_name is not None and task_name == "s2s" and getattr(self.args, "se_decoder_input", "previous_target") == "source":
            prev_output_tokens, tgt_mask = self.speech_decoder_prenet(src_tokens, src_lengths)

        if task_name is not None and task_name == "s2c":
            alignment_layer = self.decoder.num_layers    # (no layer: s2c reads no attention weights)
        else:
            alignment_layer = -1 if target_list is None and output_type == "speech" else None
        with self._no_attention_weights(task_name == "s2c"):
            decoder_output, extra = self.decoder(
                prev_output_tokens, tgt_mask, encoder_output,
                full_context_alignment=getattr(self.args, "decoder_full_context_alignment", False), alignment_layer=alignment_layer)

        if task_name is not None and task_name == "s2c":   # (:925-928) decoder pooling
            return self.speaker_decoder_postnet(self._time_mean_btc(decoder_output), sid_target), None
        # (:936-952) speech enhancement: the post-net's outputs as a mask on / a delta to the source features (reduction factor 1)
        if task_name is not None and task_name == "s2s" and getattr(self.args, "se_predict", None) is not None:
            assert self.reduction_factor == 1, f"{self.reduction_factor} != 1"
            before_outs, after_outs, logits = self.speech_decoder_postnet(decoder_output)
            se_predict = getattr(self.args, "se_predict")
            if se_predict in ("masking", "delta"):
                before_outs, after_outs = self._se_combine(before_outs, after_outs, src_tokens, se_predict)
            elif se_predict != "target":
                raise ValueError(f"{se_predict} not in [masking, target, delta]")
            return before_outs, after_outs, logits, extra["attn"][0]
        if task_name is not None and task_name == "s2t":
            return (self.text_decoder_postnet(decoder_output), None), encoder_output
        if output_type == "text":
            return (self.text_decoder_postnet(decoder_output), None), codebook_out, encoder_output
        if target_list is not None:
            return hubert_results, (self.speech_decoder_postnet(decoder_output) + (extra["attn"][0],))
        if tgt_live is not None:
            return self.speech_decoder_postnet(decoder_output, live=tgt_live) + (extra["attn"][0],)
        return self.speech_decoder_postnet(decoder_output) + (extra["attn"][0],)

    # ---- inference entry points (speecht5.py:1112-1249) ----
    def forward_encoder_torchscript(self, net_input: Dict[str, Tensor]):
        enc_in = {k: v for k, v in net_input.items() if k != "prev_output_tokens" and k != "task_name"}
        return self.forward_encoder(**enc_in)

    def forward_encoder(self, source, padding_mask=None):
        encoder_input, encoder_padding_mask = self.speech_encoder_prenet(source, padding_mask=padding_mask, mask=False)
        return self.encoder(encoder_input, encoder_padding_mask)

    # ---- length-exact batched speech encoding: every row of a right-padded batch gets what it would get alone ----
    ROWS_BYTE_BUDGET = 2 << 30   # bytes of conv layer 0's output per chunk (DESIGN.md "Length-exact batched speech encoding")

    @staticmethod
    def _row_lengths(source, padding_mask, src_lengths):
        """The rows' sample counts as a host list: `src_lengths` (list or tensor) when given, else from `padding_mask`; no mask =
        every row is full.  The counts and the suffix test are a handful of bool reductions where the mask lives (on the device for
        a device mask: no [B, S] copy to the host) and reach the host in ONE read of B + 1 integers, remembered on the mask tensor
        (as `_st5_host` is) for a caller that passes the same tensor again."""
        B, S = source.shape
        if src_lengths is not None:
            return [int(v) for v in (src_lengths.tolist() if torch.is_tensor(src_lengths) else src_lengths)]
        if padding_mask is None:
            return [S] * B
        n = getattr(padding_mask, "_st5_row_lengths", None)
        if n is None:
            if tuple(padding_mask.shape) != (B, S):
                raise ValueError(f"padding_mask {tuple(padding_mask.shape)} does not match source {(B, S)}")
            pm = padding_mask.bool()
            # right-padded = never a valid sample after a padded one: pm[:, t] implies pm[:, t + 1]
            suffix = (pm[:, 1:] | ~pm[:, :-1]).all()
            *n, ok = torch.cat([(~pm).sum(1), suffix.long().view(1)]).tolist()
            if not ok:
                raise ValueError("padding_mask is not a suffix per row: the rows path takes right-padded batches only")
            padding_mask._st5_row_lengths = n
        return n

    def _plan_row_chunks(self, n, max_samples):
        """Rows in order into chunks whose padded sample count B_chunk * n_max stays within `max_samples`; default: conv layer 0's
        output of the chunk within ROWS_BYTE_BUDGET and below 2^31 elements.  A row that is over the limit alone goes alone."""
        C0, k0, s0 = self.speech_encoder_prenet.feature_extractor.conv_layers_infos[0]
        hard = (2 ** 31 - 1) // C0                                         # frames of layer 0 per chunk
        if max_samples is None:
            frames = min(hard, self.ROWS_BYTE_BUDGET // (C0 * torch.empty(0, dtype=Fn.compute_dtype()).element_size()))
        else:
            frames = min(hard, max(1, (int(max_samples) - k0) // s0 + 1))
        chunks, cur, cur_max = [], [], 0
        for b, v in enumerate(n):
            L0 = max((v - k0) // s0 + 1, 0)
            if L0 > hard:
                raise ValueError(f"row {b}: {v} samples give {L0} x {C0} activations in conv layer 0, beyond 2^31 elements")
            m = max(cur_max, L0)
            if cur and (len(cur) + 1) * m > frames:
                chunks.append(cur)
                cur, m = [], L0
            cur.append(b)
            cur_max = m
        chunks.append(cur)
        return chunks

    def _forward_encoder_rows(self, source, padding_mask=None, src_lengths=None, max_samples=None):
        n = self._row_lengths(source, padding_mask, src_lengths)
        pre = self.speech_encoder_prenet
        xs, masks, T = [], [], [pre._frames(v) for v in n]
        for rows in self._plan_row_chunks(n, max_samples):
            nm = max(n[b] for b in rows)
            x, m = pre.forward_rows(source[rows[0]:rows[-1] + 1, :nm], [n[b] for b in rows])
            xs.append(x); masks.append(m)
        Tm = max(T)
        if len(xs) > 1:
            x = xs[0].new_zeros(len(n), Tm, xs[0].size(2))
            mask = torch.ones(len(n), Tm, dtype=torch.bool, device=x.device)
            b0 = 0
            for xc, mc in zip(xs, masks):
                x[b0:b0 + xc.size(0), :xc.size(1)] = xc
                mask[b0:b0 + xc.size(0), :xc.size(1)] = mc
                b0 += xc.size(0)
        else:
            x, mask = xs[0], masks[0]
        return self.encoder(x, mask), T

    def forward_encoder_rows(self, source, padding_mask=None, src_lengths=None, max_samples=None):
        """forward_encoder for a right-padded batch in which each row gets what it would get ALONE (inference, eval mode): the same
        dict, `encoder_out` [T_max, B, C] and `encoder_padding_mask` [B, T_max] with T_max the longest row's frame count and row b
        valid for t < T_b = frames(n_b).  The speech front end runs per chunk of rows (_plan_row_chunks; `max_samples` overrides the
        byte budget as a limit on a chunk's padded samples B_chunk * n_max), the encoder once over all rows."""
        return self._forward_encoder_rows(source, padding_mask, src_lengths, max_samples)[0]

    def forward_text_encoder(self, src_tokens):
        encoder_input, encoder_padding_mask = self.text_encoder_prenet(src_tokens)
        return self.encoder(encoder_input, encoder_padding_mask)

    def forward_decoder(self, tokens, encoder_out, incremental_state):
        """`tokens` is the whole prefix (as fairseq's SequenceGenerator passes it).  With a state dict (inference) only
        the newest token is embedded and run through the decoder, whose layers keep their keys/values in the state."""
        prev_output_tokens, tgt_mask, incremental_state = self.text_decoder_prenet(tokens, incremental_state)
        decoder_output, extra = self.decoder(prev_output_tokens, tgt_mask, encoder_out=encoder_out,
                                             incremental_state=incremental_state)
        out = self.text_decoder_postnet(decoder_output)
        if incremental_state is not None:
            out = out[:, -1:]
        return out, extra

    @staticmethod
    def _se_combine(before_outs, after_outs, src_tokens, se_predict):
        """sigmoid(outs) * src_tokens (masking) or outs - src_tokens (delta) for both post-net outputs in one launch (st5_se_predict_*).
        src_tokens broadcasts against the outputs as in the reference's torch expression; a shape that does not (or that would
        enlarge the outputs) raises, before any kernel sees it."""
        if src_tokens is None:
            raise TypeError("--se-predict masking / delta needs src_tokens (the source features) in net_input")
        shape = tuple(before_outs.shape)
        if tuple(torch.broadcast_shapes(shape, tuple(src_tokens.shape))) != shape:
            raise RuntimeError(f"src_tokens {tuple(src_tokens.shape)} does not broadcast to the decoder output {shape}")
        src = Fn.as_float(src_tokens).expand(shape)
        mode = Fn.SE_MASKING if se_predict == "masking" else Fn.SE_DELTA
        return Fn.se_predict(Fn.as_float(before_outs), Fn.as_float(after_outs), src, mode)

    def _zero_decoder_input(self, prev_output_tokens):
        """Zero decoder input [B, T, C] in the compute dtype (s2c uses a zero vector as [CLS]) and the pre-net's padding mask."""
        B, T = prev_output_tokens.shape
        x = torch.zeros(B, T, self.args.decoder_embed_dim, dtype=Fn.compute_dtype(), device=prev_output_tokens.device)
        return x, prev_output_tokens.eq(self.text_decoder_prenet.padding_idx)

    @contextlib.contextmanager
    def _no_attention_weights(self, on=True):
        """s2c reads no attention weights.  In eval every decoder layer would otherwise materialise its cross-attention
        probabilities (`need_attn`), the unfused path, whose softmax takes at most 4096 keys: a 160 s utterance has 7999.  With the
        alignment layer past the last one and need_attn off, the one query stays on the flash kernels in bf16."""
        layers = list(getattr(self.decoder, "layers", None) or []) if on else []
        old = [layer.need_attn for layer in layers]
        for layer in layers:
            layer.need_attn = False
        try:
            yield
        finally:
            for layer, v in zip(layers, old):
                layer.need_attn = v

    @staticmethod
    def _time_mean_btc(x):
        """x.mean(1) of [B, T, C] as fp32 [B, C]: a view for the one-position decoder input of s2c, else st5_time_mean."""
        if x.size(1) == 1:
            return Fn.as_float(x[:, 0])
        return Fn.time_mean(x.transpose(0, 1))

    @torch.no_grad()
    def generate_class(self, source, prev_output_tokens, exact_rows=False, **kwargs):
        """speecht5.py:1171-1186: encoder, the zeroed decoder input, decoder, speaker head on the decoder output's time mean; int64
        classes [B].  Decoder pooling whatever --sid-pooling-layer says (as the reference).  `exact_rows`: encode through
        forward_encoder_rows, so that a row's class does not depend on what else is in its batch (off: the reference's padded batch)."""
        enc = self.forward_encoder_rows if exact_rows else self.forward_encoder
        encoder_out = enc(source, padding_mask=kwargs["padding_mask"])
        x, tgt_mask = self._zero_decoder_input(prev_output_tokens)
        with self._no_attention_weights():
            decoder_output, _ = self.decoder(x, tgt_mask, encoder_out=encoder_out, alignment_layer=self.decoder.num_layers)
        decoder_out, _ = self.speaker_decoder_postnet(self._time_mean_btc(decoder_output))
        return decoder_out.argmax(1)

    def set_num_updates(self, num_updates):
        for m in self.modules():
            if m is not self and hasattr(m, "set_num_updates"):
                m.set_num_updates(num_updates)
        self.num_updates = num_updates

    @torch.no_grad()
    def generate_speech(self, source=None, src_tokens=None, spkembs=None, **kwargs):
        assert source is not None or src_tokens is not None
        threshold = kwargs.get("threshold", 0.5)
        minlenratio = kwargs.get("threshold", 0.0)  # (sic) the reference reads "threshold" for all three (:1191-1201)
        if source is None:
            assert src_tokens.size(0) == 1
            encoder_out = self.forward_text_encoder(src_tokens)
            maxlenratio = kwargs.get("threshold", 20.0)
        else:
            assert source.size(0) == 1
            encoder_out = self.forward_encoder(source, padding_mask=kwargs["padding_mask"])
            maxlenratio = kwargs.get("threshold", 10.0)
        T_in = encoder_out["encoder_out"][0].size(0)
        maxlen = int(T_in * maxlenratio / self.reduction_factor)
        minlen = int(T_in * minlenratio / self.reduction_factor)
        odim = self.speech_decoder_postnet.odim
        idx = 0
        ys = encoder_out["encoder_out"][0].new_zeros(1, 1, odim, dtype=torch.float32)
        outs, probs, attns = [], [], []
        post = self.speech_decoder_postnet
        incremental_states = {}
        while True:
            idx += 1
            decoder_in, _ = self.speech_decoder_prenet(ys, spkembs=spkembs)
            z, extra = self.decoder(decoder_in[:, -1:], None, encoder_out, incremental_states, alignment_layer=-1)
            zl = Fn.as_compute(z[:, -1:].contiguous())
            both = Fn.as_float(Fn.linear(zl, [post.feat_out.weight, post.prob_out.weight], [post.feat_out.bias, post.prob_out.bias]))
            nf = post.feat_out.weight.shape[0]
            outs += [both[0, 0, :nf].view(self.reduction_factor, odim)]
            probs += [torch.sigmoid(both[0, 0, nf:])]
            ys = torch.cat((ys, outs[-1][-1].view(1, 1, odim)), dim=1)
            attns.append(torch.stack([att_l[0, :, -1:] for att_l in extra["attn"][0]], dim=0) if isinstance(extra["attn"][0], list)
                         else extra["attn"][0][:, -1:].unsqueeze(0))
            if int(sum(probs[-1] >= threshold)) > 0 or idx >= maxlen:
                if idx < minlen:
                    continue
                mel = torch.cat(outs, dim=0).unsqueeze(0)  # (1, L, odim)
                if post.postnet is not None:
                    mel = post.postnet(Fn.as_compute(mel.contiguous()))   # fp32: mel + post-net residual (fused in the last BatchNorm kernel)
                mel = mel.squeeze(0)
                probs = torch.cat(probs, dim=0)
                attn = torch.cat(attns, dim=2)
                break
        if mel.size(0) == maxlen:
            logging.warning("output length reaches maximum length")
        return mel, probs, attn

    # ---- batched speech synthesis: generate_speech for B utterances at once, each row with its own stopping step ----
    TTS_POLL_STEPS = 8   # decode steps between two reads of the active-row count (at most this many - 1 idle steps per call)

    def _encode_rows(self, source, src_tokens, padding_mask):
        """Encoder output of B utterances as one padded batch: (encoder_out dict with [S_max, B, C] and a [B, S_max] key-padding
        mask, per-row encoder lengths T_b as a host list).  Text rows run as one padded batch (position-wise or key-masked); speech
        rows through the length-exact batched front end (forward_encoder_rows: conv layer 0's GroupNorm, the frame mask and the
        convolutional positional embedding follow each row's own length), so each row is what forward_encoder gives for it alone.
        A model in training mode (span mask / dropout semantics of forward_encoder, which the rows path does not have) keeps the
        per-clip loop on the unpadded clips."""
        if source is None:
            enc = self.forward_text_encoder(src_tokens)
            pad = src_tokens.eq(self.text_encoder_prenet.padding_idx)
            return enc, (~pad).sum(1).tolist()
        if not self.speech_encoder_prenet.training:
            return self._forward_encoder_rows(source, padding_mask)
        B = source.size(0)
        n = [source.size(1)] * B if padding_mask is None else (~padding_mask.bool()).sum(1).tolist()
        outs = []
        for b in range(B):
            pm = padding_mask[b:b + 1, :n[b]] if padding_mask is not None else source.new_zeros(1, n[b], dtype=torch.bool)
            outs.append(self.forward_encoder(source[b:b + 1, :n[b]], padding_mask=pm)["encoder_out"][0])   # [T_b, 1, C]
        T = [int(o.size(0)) for o in outs]
        S = max(T)
        x = outs[0].new_zeros(S, B, outs[0].size(2))
        for b, o in enumerate(outs):
            x[:T[b], b] = o[:, 0]
        mask = torch.arange(S, device=x.device)[None, :] >= torch.tensor(T, device=x.device)[:, None]
        return {"encoder_out": [x], "encoder_padding_mask": [mask]}, T

    def _decode_rows(self, source, src_tokens, spkembs, padding_mask, need_attn, **kwargs):
        """The decode loop of generate_speech_batch / synthesize_batch: (mel_rec fp32 [B, cap * r, odim], prob_rec fp32 [B, cap * r],
        rec = the attention record [B, layers, H, cap, S] or None, steps per row as a host list, encoder lengths T_b)."""
        assert source is not None or src_tokens is not None
        encoder_out, T_in = self._encode_rows(source, src_tokens, padding_mask)
        r = self.reduction_factor
        threshold, minlen, maxlen, cap = tts_row_limits(T_in, r, source is None, **kwargs)
        enc = encoder_out["encoder_out"][0]
        S, B = enc.size(0), enc.size(1)
        dev, dtype = enc.device, Fn.compute_dtype()
        post, pre, dec = self.speech_decoder_postnet, self.speech_decoder_prenet, self.decoder
        odim = post.odim
        C = self.args.decoder_embed_dim
        layers = list(dec.layers)
        H = layers[0].self_attn.num_heads
        hd = C // H
        # decode state: per layer a slot cache [B, cap, 2C] (identity ancestry) and this layer's view of the attention record
        anc = torch.arange(B, dtype=torch.int32, device=dev).unsqueeze(1).expand(B, cap).contiguous()
        ws = Fn.lm_decode_attn_ws(B, cap, H, hd, dev)
        rec = torch.empty(B, len(layers), H, cap, S, dtype=torch.float32, device=dev) if need_attn else None
        state = {"layers": [{"slots": torch.empty(B, cap, 2 * C, dtype=dtype, device=dev), "anc": anc, "t": 0, "ws": ws,
                             "rec": rec[:, l] if rec is not None else None} for l in range(len(layers))]}
        incremental_states = {dec._CACHE_KEY: state}
        i32 = dict(dtype=torch.int32, device=dev)
        minlen_d, maxlen_d = torch.tensor(minlen, **i32), torch.tensor(maxlen, **i32)
        done, steps, active = torch.zeros(B, **i32), torch.zeros(B, **i32), torch.zeros(1, **i32)
        mel_rec = torch.empty(B, cap * r, odim, dtype=torch.float32, device=dev)
        prob_rec = torch.empty(B, cap * r, dtype=torch.float32, device=dev)
        nxt = torch.zeros(B, odim, dtype=dtype, device=dev)
        host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        ev = torch.cuda.Event()
        pre.decoder_prenet[1].pe(cap, dev)   # (the PE table once, for every position of the loop)
        wf = [post.feat_out.weight, post.prob_out.weight]
        bf = [post.feat_out.bias, post.prob_out.bias]
        self.tts_polls = 0
        for idx in range(1, cap + 1):
            decoder_in, _ = pre(nxt.view(B, 1, odim), spkembs=spkembs, pos_offset=idx - 1)
            z, _ = dec(decoder_in, None, encoder_out, incremental_states, alignment_layer=-1)
            y = Fn.as_float(Fn.linear(Fn.as_compute(z.reshape(B, C)), wf, bf))
            Fn.tts_step_tail(y, r, odim, minlen_d, maxlen_d, done, steps, idx, threshold, mel_rec, prob_rec, nxt, active)
            if idx % self.TTS_POLL_STEPS == 0 and idx < cap:
                host.copy_(active, non_blocking=True)
                ev.record()
                ev.synchronize()
                self.tts_polls += 1
                if int(host[0]) == 0:
                    break
        return mel_rec, prob_rec, rec, steps.tolist(), T_in

    def _decode_rows_mode(self, decode, source, src_tokens, spkembs, padding_mask, need_attn, **kwargs):
        """_decode_rows in the requested mode: "eager" (the loop above), "device" (every kernel of a step reads the step index from
        device memory: speecht5_amd/tts_graph.py) or "graph" (that step captured once and replayed).  Records what ran in
        tts_decode_mode / tts_polls / tts_device_steps / tts_graph_replays."""
        from . import tts_graph
        if decode not in tts_graph.DECODE_MODES:
            raise ValueError(f"decode must be one of {tts_graph.DECODE_MODES}, got {decode!r}")
        self.tts_decode_mode, self.tts_device_steps, self.tts_graph_replays = decode, 0, 0
        if decode == "eager":
            return self._decode_rows(source, src_tokens, spkembs, padding_mask, need_attn, **kwargs)
        return tts_graph.decode_rows(self, source, src_tokens, spkembs, padding_mask, need_attn, decode, **kwargs)

    @torch.no_grad()
    def generate_speech_batch(self, source=None, src_tokens=None, spkembs=None, padding_mask=None, need_attn=True, decode="eager",
                              **kwargs):
        """generate_speech for B utterances in one decode loop.  Returns B tuples (mel [L_b, odim], probs [L_b], attn
        [decoder_layers, H, L_b / r, S_b] or None) in row order, each as generate_speech returns it for that row alone.  Text rows
        are right-padded (TextToSpeechCollater); speech rows come with `padding_mask`.  Row b stops at the first step idx >= minlen_b
        at which one of its r stop probabilities reaches `threshold` or idx >= maxlen_b; rows that stopped keep computing (their
        records are final) until the host sees no active row, every TTS_POLL_STEPS steps.  decode: "eager" (default), or the
        device-stepped loop on the skinny-M GEMM kernel launched kernel by kernel ("device") or replayed from a HIP graph ("graph")."""
        mel_rec, prob_rec, rec, L, T_in = self._decode_rows_mode(decode, source, src_tokens, spkembs, padding_mask, need_attn, **kwargs)
        post, r = self.speech_decoder_postnet, self.reduction_factor
        out = []
        for b in range(len(L)):
            mel = mel_rec[b, :L[b] * r].unsqueeze(0)
            if post.postnet is not None:
                mel = post.postnet(Fn.as_compute(mel.contiguous()))
            attn = rec[b, :, :, :L[b], :T_in[b]].contiguous() if rec is not None else None
            out.append((mel.squeeze(0), prob_rec[b, :L[b] * r].clone(), attn))
        return out

    @torch.no_grad()
    def synthesize_batch(self, source=None, src_tokens=None, spkembs=None, padding_mask=None, vocoder=None, need_attn=False,
                         max_frames=None, decode="eager", **kwargs):
        """B texts (or B source clips) in, B waveforms out: the decode loop of generate_speech_batch, then the mel post-net and the
        HiFi-GAN `vocoder` over packed sequences (speecht5_amd/ragged.py) instead of once per row.  Returns B tuples (wav fp32
        [hop * L_b] or None without a vocoder, mel [L_b, odim], probs [L_b], attn or None), each row what generate_speech, the
        post-net and vocoder.forward give for that row alone.  The mel records are packed on the device straight from the decode
        loop's record; one layout (the vocoder's gap when there is one) serves the post-net and the vocoder.  Rows go in order into
        chunks of at most `max_frames` mel frames (default: the vocoder's byte budget).  decode: as in generate_speech_batch."""
        from . import ragged
        mel_rec, prob_rec, rec, steps, T_in = self._decode_rows_mode(decode, source, src_tokens, spkembs, padding_mask, need_attn, **kwargs)
        post, r = self.speech_decoder_postnet, self.reduction_factor
        B, rows_per, odim = mel_rec.shape
        lengths = [n * r for n in steps]
        gap = max(ragged.postnet_gap(post.postnet) if post.postnet is not None else 0, vocoder.ragged_gap() if vocoder is not None else 0)
        if vocoder is not None:
            max_frames = min(vocoder.default_max_frames() if max_frames is None else int(max_frames), vocoder.frame_limit())
            hop = vocoder._packed_rate()
        src = mel_rec.view(B * rows_per, odim)
        wavs, mels = [None] * B, [None] * B
        for rows in ragged.plan_chunks(lengths, gap, max_frames):
            lay = ragged.PackedLayout([lengths[b] for b in rows], gap, [b * rows_per for b in rows], src.device)
            if post.postnet is not None:
                after = Fn.postnet_ragged(lay.pack_rows(src, Fn.compute_dtype()), post.postnet.postnet, lay)   # fp32 [T, odim]
            else:
                after = lay.pack_rows(src, torch.float32)
            _, per_row = lay.unpack_rows(after, odim)
            for b, m in zip(rows, per_row):
                mels[b] = m
            if vocoder is not None:
                _, per_row = lay.unpack_rows(vocoder.forward_packed(Fn.to_compute(after), lay), hop)
                for b, w in zip(rows, per_row):
                    wavs[b] = w.reshape(-1)
        out = []
        for b in range(B):
            attn = rec[b, :, :, :steps[b], :T_in[b]].contiguous() if rec is not None else None
            out.append((wavs[b], mels[b], prob_rec[b, :lengths[b]].clone(), attn))
        return out

    # ---- streaming synthesis: a fixed set of decoder rows, finished rows refilled in the decode loop (speecht5_amd/tts_stream.py) ----
    def generate_speech_stream(self, requests, *, rows, max_src_len, decode="graph", need_attn=False, **kwargs):
        """generate_speech for utterances as they arrive.  requests: an iterable of (key, src_tokens [n] or source waveform [n],
        spkembs [D]); yields (key, mel, probs, attn), each what generate_speech_batch returns for a row, in completion order (rows
        that finish at the same poll in row order).  `rows` decoder rows are stepped by one program ("device": kernel by kernel,
        "graph": captured once and replayed); every TTS_POLL_STEPS steps the finished rows are copied out and handed to the next
        waiting utterances, which were encoded alone, as generate_speech encodes them.  max_src_len: the most encoder positions an
        utterance may have (a longer one is refused by key when the stream ends; the others complete).  `threshold` and the length
        ratios are read per row by tts_row_limits."""
        from . import tts_stream
        post = self.speech_decoder_postnet

        def finish(raw):
            out = []
            for key, mel, probs, attn in raw:
                mel = mel.unsqueeze(0)
                if post.postnet is not None:
                    mel = post.postnet(Fn.as_compute(mel.contiguous()))
                out.append((key, mel.squeeze(0), probs, attn))
            return out
        return tts_stream.run_stream(self, requests, rows, max_src_len, decode, need_attn, finish, **kwargs)

    def synthesize_stream(self, requests, *, rows, max_src_len, vocoder=None, decode="graph", max_frames=None, **kwargs):
        """generate_speech_stream through the mel post-net and the HiFi-GAN `vocoder`: yields (key, wav fp32 [hop * L] or None without
        a vocoder, mel [L, odim], probs [L]).  The rows that completed at one poll go together through the packed post-net / vocoder
        path of synthesize_batch."""
        from . import ragged, tts_stream
        post = self.speech_decoder_postnet

        def finish(raw):
            if not raw:
                return []
            odim = raw[0][1].shape[1]
            lengths = [m.shape[0] for _, m, _, _ in raw]
            starts = [sum(lengths[:i]) for i in range(len(raw))]
            src = torch.cat([m for _, m, _, _ in raw], 0)
            gap = max(ragged.postnet_gap(post.postnet) if post.postnet is not None else 0, vocoder.ragged_gap() if vocoder is not None else 0)
            mf = max_frames
            if vocoder is not None:
                mf = min(vocoder.default_max_frames() if max_frames is None else int(max_frames), vocoder.frame_limit())
                hop = vocoder._packed_rate()
            wavs, mels = [None] * len(raw), [None] * len(raw)
            for idx in ragged.plan_chunks(lengths, gap, mf):
                lay = ragged.PackedLayout([lengths[b] for b in idx], gap, [starts[b] for b in idx], src.device)
                if post.postnet is not None:
                    after = Fn.postnet_ragged(lay.pack_rows(src, Fn.compute_dtype()), post.postnet.postnet, lay)
                else:
                    after = lay.pack_rows(src, torch.float32)
                _, per_row = lay.unpack_rows(after, odim)
                for b, m in zip(idx, per_row):
                    mels[b] = m
                if vocoder is not None:
                    _, per_row = lay.unpack_rows(vocoder.forward_packed(Fn.to_compute(after), lay), hop)
                    for b, w in zip(idx, per_row):
                        wavs[b] = w.reshape(-1)
            return [(raw[b][0], wavs[b], mels[b], raw[b][2]) for b in range(len(raw))]
        return tts_stream.run_stream(self, requests, rows, max_src_len, decode, False, finish, **kwargs)

    # ---- checkpoint compatibility (speecht5.py:1022-1058): non-strict per-submodule load ----
    def load_state_dict(self, state_dict, strict=True, model_cfg=None, args=None):
        """Never strict (as the reference): a checkpoint trained with another dictionary loses its dictionary-sized tensors
        (text pre/post-nets, CTC projection: speecht5.py:1036-1051), every other tensor whose shape differs is dropped with
        a warning, and each top-level module then takes what the checkpoint has for it."""
        state_dict = dict(state_dict)
        self.upgrade_state_dict_named(state_dict, "")
        post = getattr(self, "text_decoder_postnet", None)
        key = "text_decoder_postnet.output_projection.weight"
        if post is not None and key in state_dict and state_dict[key].size(0) != post.output_projection.weight.size(0):
            logger.warning(f"dictionary size differs (model {post.output_projection.weight.size(0)} vs checkpoint "
                           f"{state_dict[key].size(0)}): dictionary-sized modules keep their initialisation")
            for k in [k for k in state_dict if k.startswith(("encoder.proj", "text_encoder_prenet", "text_decoder_prenet",
                                                             "text_decoder_postnet"))]:
                state_dict.pop(k)
        own = self.state_dict()
        for k in list(state_dict.keys()):
            if k in own and own[k].shape != state_dict[k].shape:
                logger.warning(f"dropping {k}: checkpoint shape {tuple(state_dict[k].shape)} != model {tuple(own[k].shape)}")
                state_dict.pop(k)
        return super().load_state_dict(state_dict, strict=False)

    def upgrade_state_dict_named(self, state_dict, name):
        """Old-checkpoint fixes of the fairseq lineage, applied to the keys in place: fused `in_proj_weight / in_proj_bias`
        of attention blocks are split into q/k/v projections (multihead_attention.py:493-522); the numbered decoder layer
        norms `layer_norms.{0,1,2}` get their names (decoder.py:290-300)."""
        for k in list(state_dict.keys()):
            if k.endswith("in_proj_weight") or k.endswith("in_proj_bias"):
                base, kind = k.rsplit("in_proj_", 1)
                w = state_dict.pop(k)
                n = w.shape[0] // 3
                for i, pn in enumerate(("q_proj", "k_proj", "v_proj")):
                    state_dict[f"{base}{pn}.{kind}"] = w[i * n:(i + 1) * n]
        names = {"0": "self_attn_layer_norm", "1": "encoder_attn_layer_norm", "2": "final_layer_norm"}
        for k in list(state_dict.keys()):
            if ".layer_norms." in k and k.startswith((name + "decoder.") if name else "decoder."):
                head, tail = k.split(".layer_norms.", 1)
                idx, rest = tail.split(".", 1)
                if idx in names:
                    state_dict[f"{head}.{names[idx]}.{rest}"] = state_dict.pop(k)
        return state_dict

    def prune_modules(self, modules_filter=None):
        """Drop the sub-modules a fine-tuning task never uses (speecht5.py:1060-1110): `s2s`, `t2s`, `s2c`, `s3prl`."""
        if modules_filter is None:
            return

        def drop(*names):
            for n in names:
                if n in self._modules:
                    del self._modules[n]
                    if n == "quantizer":
                        self.use_codebook = False

        def drop_decoder_stack():
            for n in ("dropout_module", "layers", "layer_norm"):
                if n in self.decoder._modules:
                    del self.decoder._modules[n]

        # (the reference deletes `speech_encoder_postnet`, an attribute that does not exist -- the HuBERT head is registered as
        # `hubert_layer` -- so the head SURVIVES pruning there and its keys stay in fine-tuned checkpoints: kept here too, for
        # byte-compatible state dicts)
        common = ("speech_encoder_postnet", "projection", "quantizer")
        if modules_filter == "s2c":
            pooling = getattr(self.args, "sid_pooling_layer", "decoder")
            drop("text_encoder_prenet", "speech_decoder_postnet", "text_decoder_postnet", *common)
            if pooling != "decoder-las":
                drop("speech_decoder_prenet")
            if pooling.startswith("encoder") or getattr(self.args, "sid_decoder_speaker", False):
                drop_decoder_stack()
                drop("text_decoder_prenet")
        elif modules_filter == "s2s":
            drop("speaker_decoder_postnet", "text_encoder_prenet", "text_decoder_prenet", "text_decoder_postnet", *common)
        elif modules_filter == "t2s":
            drop("speaker_decoder_postnet", "speech_encoder_prenet", "text_decoder_prenet", "text_decoder_postnet", *common)
        elif modules_filter == "s3prl":
            drop_decoder_stack()
            drop("speaker_decoder_postnet", "text_decoder_prenet", "text_decoder_postnet", "speech_decoder_prenet",
                 "speech_decoder_postnet", *common)
        else:
            raise ValueError(f"unknown modules filter {modules_filter!r}")
        if getattr(self.encoder, "proj", None) is not None:
            self.encoder.proj = None


# ---- architectures (speecht5.py:1252-1447) ----
@register_model_architecture(model_name="t5_transformer", arch_name="t5_transformer")
def base_architecture(args):
    def d(name, value):
        setattr(args, name, getattr(args, name, value))

    d("bert_init", False)
    d("encoder_embed_dim", 768)
    d("encoder_ffn_embed_dim", 768 * 4)
    d("encoder_layers", 12)
    d("encoder_attention_heads", 12)
    d("encoder_normalize_before", False)
    d("decoder_embed_dim", args.encoder_embed_dim)
    d("decoder_ffn_embed_dim", args.encoder_ffn_embed_dim)
    d("decoder_layers", 6)
    d("decoder_attention_heads", 12)
    d("decoder_normalize_before", False)
    d("dropout", 0.1)
    d("attention_dropout", args.dropout)
    d("activation_dropout", args.dropout)
    d("activation_fn", "gelu")
    d("decoder_layerdrop", 0.0)
    d("decoder_output_dim", args.decoder_embed_dim)
    d("decoder_input_dim", args.decoder_embed_dim)
    d("encoder_layerdrop", 0)
    d("max_text_positions", DEFAULT_MAX_TEXT_POSITIONS)
    d("max_speech_positions", DEFAULT_MAX_SPEECH_POSITIONS)
    d("use_batch_norm", True)
    d("enc_use_scaled_pos_enc", True)
    d("dec_use_scaled_pos_enc", True)
    d("postnet_layers", 5)
    d("postnet_chans", 256)
    d("postnet_filts", 5)
    d("postnet_dropout_rate", 0.5)
    d("dprenet_dropout_rate", 0.5)
    d("dprenet_layers", 2)
    d("dprenet_units", 256)
    d("initial_encoder_alpha", 1.0)
    d("initial_decoder_alpha", 1.0)
    d("spk_embed_integration_type", "pre")
    d("spk_embed_dim", 512)
    d("encoder_reduction_factor", 1)
    d("reduction_factor", 2)
    d("transformer_enc_positional_dropout_rate", 0.1)
    d("transformer_dec_positional_dropout_rate", 0.1)
    d("layer_norm_eps", 1e-5)
    d("no_scale_embedding", True)
    d("encoder_speech_prenet", "conv")
    d("quant_noise_pq", 0)
    d("adaptive_softmax_cutoff", None)
    d("adaptive_softmax_dropout", 0)
    d("no_token_positional_embeddings", False)
    d("adaptive_input", False)
    d("decoder_learned_pos", False)
    d("share_input_output_embed", False)
    d("share_ctc_embed", False)
    d("freeze_encoder_updates", 0)
    d("freeze_decoder_updates", 0)
    d("no_freeze_encoder_layer", None)
    d("sid_embed_dim", 128)
    d("sid_pooling_layer", "decoder")
    d("softmax_scale", 1)
    d("softmax_margin", 0)
    d("softmax_easy_margin", False)
    d("modules_filter", None)
    d("conv_pos", 128)
    d("conv_pos_groups", 16)
    d("target_glu", False)
    d("logit_temp", 0.1)
    d("final_dim", 256)
    d("untie_final_proj", True)
    d("feature_grad_mult", 0.1)
    d("use_sent_enc_layer", True)
    d("extractor_mode", "default")
    d("conv_feature_layers", "[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2")
    d("conv_bias", False)
    d("hubert_mask_length", 10)
    d("mask_prob", 0.0)
    d("mask_selection", "static")
    d("mask_other", 0)
    d("no_mask_overlap", False)
    d("mask_min_space", 1)
    d("mask_channel_length", 10)
    d("mask_channel_prob", 0.0)
    d("mask_channel_selection", "static")
    d("mask_channel_other", 0)
    d("no_mask_channel_overlap", False)
    d("mask_channel_min_space", 1)
    d("skip_masked", False)
    d("skip_nomask", False)
    d("use_conv_pos", False)
    d("use_sinc_pos", False)
    d("use_codebook", False)
    d("latent_vars", 100)
    d("latent_groups", 2)
    d("latent_dim", 0)
    d("latent_temp", (2, 0.5, 0.999995))
    d("quantizer_depth", 1)
    d("quantizer_factor", 3)
    d("codebook_prob", 0.5)
    d("relative_position_embedding", False)
    d("num_buckets", 320)
    d("max_distance", 1280)
    d("encoder_max_relative_position", 160)
    d("decoder_max_relative_position", 160)


@register_model_architecture("t5_transformer", "t5_transformer_base")
def t5_transformer_base(args):
    def d(name, value):
        setattr(args, name, getattr(args, name, value))
    d("use_conv_pos", True)
    d("use_sinc_pos", True)
    d("layernorm_embedding", False)
    d("encoder_normalize_before", False)
    d("decoder_normalize_before", False)
    d("layer_norm_first", False)
    d("relative_position_embedding", True)
    d("dropout", 0.1)
    d("activation_dropout", 0.0)
    d("attention_dropout", 0.1)
    d("encoder_layerdrop", 0.05)
    d("decoder_layerdrop", 0.05)
    d("mask_prob", 0.80)
    base_architecture(args)


@register_model_architecture("t5_transformer", "t5_transformer_large")
def t5_transformer_large(args):
    def d(name, value):
        setattr(args, name, getattr(args, name, value))
    d("use_conv_pos", True)
    d("use_sinc_pos", True)
    d("encoder_normalize_before", False)
    d("decoder_normalize_before", True)
    d("layer_norm_first", True)
    d("relative_position_embedding", True)
    d("dropout", 0.0)
    d("activation_dropout", 0.0)
    d("attention_dropout", 0.0)
    d("encoder_layerdrop", 0.0)
    d("decoder_layerdrop", 0.0)
    d("encoder_embed_dim", 1024)
    d("encoder_layers", 24)
    d("decoder_layers", 6)
    d("encoder_ffn_embed_dim", 4096)
    d("encoder_attention_heads", 16)
    d("decoder_attention_heads", 16)
    d("feature_grad_mult", 1.0)
    d("extractor_mode", "layer_norm")
    d("final_dim", 768)
    d("mask_prob", 0.80)
    base_architecture(args)


@register_model_architecture("t5_transformer", "t5_transformer_base_asr")
def t5_transformer_base_asr(args):
    def d(name, value):
        setattr(args, name, getattr(args, name, value))
    d("use_conv_pos", True)
    d("use_sinc_pos", True)
    d("encoder_normalize_before", False)
    d("decoder_normalize_before", False)
    d("layer_norm_first", False)
    d("relative_position_embedding", True)
    d("dropout", 0.1)
    d("activation_dropout", 0.1)
    d("attention_dropout", 0.1)
    d("feature_grad_mult", 0.0)
    d("encoder_layerdrop", 0.1)
    d("decoder_layerdrop", 0.1)
    d("mask_prob", 0.75)
    d("mask_selection", "static")
    d("mask_channel_length", 64)
    d("mask_channel_prob", 0.5)
    d("mask_channel_selection", "static")
    d("max_text_positions", 600)
    base_architecture(args)
