"""The shallow-fusion language model of ASR decoding (arch `transformer_lm_t5`, SpeechT5/speecht5/models/t5_transformer_lm.py:18-27)
on the HIP kernels, with an incremental decode path made for beam search.

fairseq is not part of the reference tree, so this is a RESTATEMENT of fairseq's `transformer_lm` model (TransformerLanguageModel
with a TransformerDecoder without encoder attention) as `base_lm_architecture` fills it in for `transformer_lm_t5`:
  x = embed_scale * embed_tokens[tok] + sinusoidal[pos],  pos = cumsum(tok != pad) * (tok != pad) + pad,  embed_scale = sqrt(d)
  (fairseq SinusoidalPositionalEmbedding, vendored verbatim at SpeechLM/modules.py:1296; the table is rebuilt larger when a
  sequence outgrows it, as fairseq's is -- a row's values do not depend on the table size);
  L pre-LN layers (decoder_normalize_before is forced on): x += out_proj(causal self-attention(LN(x))), x += fc2(act(fc1(LN(x))));
  final decoder.layer_norm; output_projection without bias, or tied to embed_tokens (share_decoder_input_output_embed).
State-dict keys are fairseq's (decoder.embed_tokens.weight, decoder.embed_positions._float_tensor, decoder.layers.{i}.*,
decoder.layer_norm.*, decoder.output_projection.weight, decoder.version).

Two ways to run it:
  forward(src_tokens): the full-prefix path, what the reference calls at every beam-search step
  (SpeechT5/speecht5/sequence_generator.py:420-425): every position through every layer (modules/transformer_layer.py's
  TransformerDecoderLayer without encoder attention, causal self-attention, key-padding mask of the pad tokens).
  init_decode / decode_step / reorder: one new position per hypothesis row and step.  Each layer keeps the projected keys and
  values of every position it has seen in a SLOT cache kv [rows_cap, Tmax, 2C]: slot (r, j) holds what row r produced at
  position j, written once (the K / V projection GEMM writes it in place).  One int32 ancestry table anc [rows, Tmax], shared by
  all layers, says which slot row r reads at position j; a beam reorder gathers that table (st5_lm_reorder) and moves no key or
  value.  Attention of the newest position: st5_lm_decode_attn (csrc/lm_decode.hip).
  device_step: the same step as a list of launches behind a device step counter (step_program.py), for the device-stepped beam
  search (beam_graph.py): the slot caches are read through the text decoder's ancestry table, there is no reorder of the LM's own.
  device_step_sents: that step with one position per sentence slot, for the beam-search stream (beam_stream.py).

Layouts it does not implement raise NotImplementedError naming the option: adaptive softmax / adaptive input, learned positions,
layernorm_embedding, post-LN layers, no_decoder_final_norm, character embeddings, decoder_input_dim != decoder_embed_dim."""
import math
from argparse import Namespace

import torch
import torch.nn as nn

from . import functional as Fn
from . import hip
from .modules.common import LayerNorm, SinusoidalPositionalEmbedding
from .modules.transformer_layer import TransformerDecoderLayer
from .step_program import append_layers
from .t5_transformer_lm import _PRESET

DEFAULT_MAX_POSITIONS = 1024   # fairseq transformer_lm: max_target_positions = tokens_per_sample (1024)


def _lm_args(args=None, **dims):
    """The transformer_lm_t5 namespace: explicit `dims` over `args` over the preset over base_lm_architecture's defaults."""
    a = Namespace(**vars(args)) if args is not None else Namespace()
    for k, v in dims.items():
        if v is not None:
            setattr(a, k, v)
    for k, v in _PRESET:
        if getattr(a, k, None) is None:
            setattr(a, k, v)
    defaults = dict(activation_dropout=0.0, relu_dropout=0.0, adaptive_softmax_cutoff=None, decoder_learned_pos=False,
                    no_token_positional_embeddings=False, share_decoder_input_output_embed=False, character_embeddings=False,
                    no_decoder_final_norm=False, adaptive_input=False, no_scale_embedding=False, layernorm_embedding=False,
                    max_target_positions=None, tokens_per_sample=DEFAULT_MAX_POSITIONS)
    for k, v in defaults.items():
        if not hasattr(a, k):
            setattr(a, k, v)
    if getattr(a, "decoder_final_norm", None) is not None:     # (base_lm_architecture's backward-compatibility spelling)
        a.no_decoder_final_norm = not a.decoder_final_norm
    for k in ("decoder_input_dim", "decoder_output_dim"):
        if getattr(a, k, None) is None:
            setattr(a, k, a.decoder_embed_dim)
    return a


def check_supported(args):
    """NotImplementedError naming the first option of `args` this model does not implement."""
    refused = [
        ("adaptive_softmax_cutoff", lambda a: a.adaptive_softmax_cutoff not in (None, "", 0)),
        ("adaptive_input", lambda a: bool(a.adaptive_input)),
        ("decoder_learned_pos", lambda a: bool(a.decoder_learned_pos)),
        ("no_token_positional_embeddings", lambda a: bool(a.no_token_positional_embeddings)),
        ("layernorm_embedding", lambda a: bool(a.layernorm_embedding)),
        ("decoder_normalize_before", lambda a: getattr(a, "decoder_normalize_before", True) is False),
        ("no_decoder_final_norm", lambda a: bool(a.no_decoder_final_norm)),
        ("character_embeddings", lambda a: bool(a.character_embeddings)),
        ("decoder_input_dim", lambda a: a.decoder_input_dim != a.decoder_embed_dim),
        ("decoder_output_dim", lambda a: a.decoder_output_dim != a.decoder_embed_dim),
        ("activation_fn", lambda a: str(a.activation_fn) not in ("gelu", "relu", "tanh", "linear")),
    ]
    for name, bad in refused:
        if bad(args):
            raise NotImplementedError(f"transformer_lm option {name}={getattr(args, name, None)!r} is not implemented by "
                                      "speecht5_amd.transformer_lm.TransformerLanguageModel")


# state-dict keys that only a refused layout writes
_REFUSED_KEYS = (("decoder.adaptive_softmax.", "adaptive_softmax_cutoff"), ("decoder.embed_positions.weight", "decoder_learned_pos"),
                 ("decoder.layernorm_embedding.", "layernorm_embedding"), ("decoder.project_in_dim.", "decoder_input_dim"),
                 ("decoder.project_out_dim.", "decoder_output_dim"), ("decoder.embed_tokens.char_embeddings", "character_embeddings"),
                 ("decoder.embed_tokens.embeddings.", "adaptive_input"))


class _LMDecoder(nn.Module):
    def __init__(self, args, vocab, pad):
        super().__init__()
        d = args.decoder_embed_dim
        self.padding_idx = pad
        self.embed_tokens = nn.Embedding(vocab, d, padding_idx=pad)
        nn.init.normal_(self.embed_tokens.weight, mean=0, std=d ** -0.5)
        with torch.no_grad():
            self.embed_tokens.weight[pad].zero_()
        self.embed_scale = 1.0 if args.no_scale_embedding else math.sqrt(d)
        self.embed_positions = SinusoidalPositionalEmbedding(d, pad)
        largs = Namespace(**vars(args))
        largs.decoder_normalize_before = True
        self.layers = nn.ModuleList([TransformerDecoderLayer(largs, no_encoder_attn=True) for _ in range(args.decoder_layers)])
        self.layer_norm = LayerNorm(d)
        self.output_projection = nn.Linear(d, vocab, bias=False)
        if args.share_decoder_input_output_embed:
            self.output_projection.weight = self.embed_tokens.weight
        else:
            nn.init.normal_(self.output_projection.weight, mean=0, std=d ** -0.5)
        self.register_buffer("version", torch.Tensor([3]))


class DecodeState:
    """Per-generate() decode state: one slot cache per layer, the ancestry table (double-buffered: the reorder gathers into the
    other buffer), the number of positions written, and the attention workspace."""

    def __init__(self, kv, anc_bufs, ws, Tmax):
        self.kv = kv
        self.bufs = anc_bufs
        self.cur = 0
        self.anc = anc_bufs[0]
        self.t = 0
        self.ws = ws
        self.Tmax = Tmax

    @property
    def rows(self):
        return self.anc.shape[0]


class TransformerLanguageModel(nn.Module):
    def __init__(self, args, vocab, pad=1):
        super().__init__()
        args = _lm_args(args)
        check_supported(args)
        self.args = args
        self.decoder = _LMDecoder(args, vocab, pad)
        self.num_heads = args.decoder_attention_heads
        self.head_dim = args.decoder_embed_dim // self.num_heads
        assert self.head_dim * self.num_heads == args.decoder_embed_dim

    # ---- construction from fairseq weights ----
    @classmethod
    def from_state_dict(cls, sd, args=None, pad=1):
        """Dims from the tensor shapes (vocabulary, width, layers, FFN width); the head count from `args` or the transformer_lm_t5
        preset.  Refuses layouts it does not implement (NotImplementedError)."""
        sd = {k: v for k, v in sd.items()}
        for prefix, option in _REFUSED_KEYS:
            if any(k.startswith(prefix) for k in sd):
                raise NotImplementedError(f"transformer_lm option {option} (state-dict key {prefix}*) is not implemented by "
                                          "speecht5_amd.transformer_lm.TransformerLanguageModel")
        if "decoder.layer_norm.weight" not in sd:
            raise NotImplementedError("transformer_lm option no_decoder_final_norm (no decoder.layer_norm in the state dict) is not "
                                      "implemented by speecht5_amd.transformer_lm.TransformerLanguageModel")
        if "decoder.version" in sd and float(sd["decoder.version"].reshape(-1)[0]) <= 2:
            raise NotImplementedError("transformer_lm option no_decoder_final_norm (decoder.version <= 2: a checkpoint from before "
                                      "the final LayerNorm) is not implemented by speecht5_amd.transformer_lm.TransformerLanguageModel")
        vocab, d = sd["decoder.embed_tokens.weight"].shape
        n_layers = 0
        while f"decoder.layers.{n_layers}.fc1.weight" in sd:
            n_layers += 1
        ffn = sd["decoder.layers.0.fc1.weight"].shape[0] if n_layers else (args.decoder_ffn_embed_dim if args else None)
        tied = "decoder.output_projection.weight" not in sd or (
            args is not None and bool(getattr(args, "share_decoder_input_output_embed", False)))
        a = _lm_args(args, decoder_embed_dim=d, decoder_layers=n_layers, decoder_ffn_embed_dim=ffn)
        a.share_decoder_input_output_embed = tied
        m = cls(a, vocab, pad)
        sd.setdefault("decoder.version", torch.Tensor([3]))
        sd.setdefault("decoder.embed_positions._float_tensor", torch.FloatTensor(1))
        if tied:
            sd["decoder.output_projection.weight"] = sd["decoder.embed_tokens.weight"]
        m.load_state_dict(sd, strict=True)
        return m

    def max_positions(self):
        return int(self.args.max_target_positions or self.args.tokens_per_sample or DEFAULT_MAX_POSITIONS)

    def _embed(self, tokens, positions):
        dec = self.decoder
        table = dec.embed_positions.table(tokens.shape[-1] + dec.padding_idx + 2, tokens.device)   # (positions <= pad + T)
        return Fn.embed_rows(dec.embed_tokens.weight, tokens, pos=table, pidx=positions, emb_scale=dec.embed_scale)

    # ---- full-prefix path ----
    def forward(self, src_tokens, src_lengths=None, **kwargs):
        """src_tokens [B, T] -> (logits [B, T, V] fp32, {"attn": [None], "inner_states": [T x B x C] * (L + 1)}), as fairseq's
        TransformerDecoder returns them (inner states: the embedding output and every layer's output, before the final norm)."""
        dec = self.decoder
        B, T = src_tokens.shape
        pad = src_tokens.eq(dec.padding_idx)
        positions = dec.embed_positions.positions(~pad)
        x = self._embed(src_tokens, positions)
        C = x.shape[-1]
        rows = x.reshape(B * T, C)
        inner = [rows]
        for layer in dec.layers:
            rows, _ = layer.forward_rows(rows, B, T, None, None, None, pad, True, False)
            inner.append(rows)
        rows = dec.layer_norm(rows)
        logits = Fn.as_float(Fn.linear(rows, dec.output_projection.weight, None)).view(B, T, -1)
        states = [Fn.as_float(r).view(B, T, C).transpose(0, 1) for r in inner]
        return logits, {"attn": [None], "inner_states": states}

    def get_normalized_probs(self, net_output, log_probs, sample=None):
        logits = net_output[0].float()
        return torch.log_softmax(logits, dim=-1) if log_probs else torch.softmax(logits, dim=-1)

    # ---- incremental path (beam search) ----
    @torch.no_grad()
    def init_decode(self, rows, max_len, anc=None):
        """Slot caches [rows, max_len, 2C] per layer in the compute dtype, the ancestry table (identity: every row reads its own
        slots) and the attention workspace -- allocated once per generate() call.
        anc: an int32 [rows, max_len] ancestry table that somebody else owns and reorders (the text decoder's, in the device-stepped
        beam search: the LM's rows are the decoder's rows with the same ancestry).  The state then holds no table of its own and is
        one for device_step; decode_step / reorder need the default."""
        dev = self.decoder.embed_tokens.weight.device
        dtype = Fn.compute_dtype()
        C = self.args.decoder_embed_dim
        kv = [torch.empty(rows, max_len, 2 * C, dtype=dtype, device=dev) for _ in self.decoder.layers]
        if anc is not None:
            if anc.dtype != torch.int32 or tuple(anc.shape) != (rows, max_len) or anc.stride(1) != 1 or anc.device != dev:
                raise ValueError(f"init_decode: anc must be an int32 [{rows}, {max_len}] table on {dev}, got {anc.dtype} "
                                 f"{tuple(anc.shape)} on {anc.device}")
            return DecodeState(kv, [anc], Fn.lm_decode_attn_ws(rows, max_len, self.num_heads, self.head_dim, dev), max_len)
        ident = torch.arange(rows, dtype=torch.int32, device=dev).unsqueeze(1).expand(rows, max_len)
        bufs = [ident.contiguous(), torch.empty(rows, max_len, dtype=torch.int32, device=dev)]
        ws = Fn.lm_decode_attn_ws(rows, max_len, self.num_heads, self.head_dim, dev)
        return DecodeState(kv, bufs, ws, max_len)

    @torch.no_grad()
    def decode_step(self, last_tokens, state):
        """last_tokens [rows]: the newest token of every hypothesis row (position state.t of a pad-free prefix, as beam search
        feeds it).  Returns logits [rows, V] of that position in the compute dtype."""
        dec = self.decoder
        p = state.t
        if p >= state.Tmax:
            raise ValueError(f"decode_step: position {p} is past the {state.Tmax} positions of this decode state")
        rows = last_tokens.numel()
        assert rows == state.rows, (rows, state.rows)
        H, hd = self.num_heads, self.head_dim
        C = H * hd
        tok = last_tokens.reshape(rows)
        pidx = torch.full((rows,), dec.padding_idx + 1 + p, dtype=torch.int32, device=tok.device)
        table = dec.embed_positions.table(p + dec.padding_idx + 2, tok.device)
        x = Fn.embed_rows(dec.embed_tokens.weight, tok, pos=table, pidx=pidx, emb_scale=dec.embed_scale)
        for layer, kv in zip(dec.layers, state.kv):
            sa = layer.self_attn
            h = layer.self_attn_layer_norm(x)
            q = Fn.linear(h, sa.q_proj.weight, sa.q_proj.bias)
            Fn.linear_into(h, [sa.k_proj.weight, sa.v_proj.weight], [sa.k_proj.bias, sa.v_proj.bias],
                           hip.operand(kv, state.Tmax * 2 * C, off=p * 2 * C), 2 * C)
            ctx = Fn.lm_decode_attn(q, kv, state.anc, p + 1, H, hd, state.ws)
            x = Fn.linear(ctx, sa.out_proj.weight, sa.out_proj.bias, residual=x)
            h = layer.final_layer_norm(x)
            x = Fn.ffn(h, x, layer.fc1, layer.fc2, layer.act, 0.0, 0.0)
        x = dec.layer_norm(x)
        state.t = p + 1
        return Fn.linear(x, dec.output_projection.weight, None)

    @torch.no_grad()
    def device_step(self, state, bs, prog):
        """The LM's share of one DEVICE-STEPPED beam search step (beam_graph.BeamDeviceDecode): appends to `prog`
        (step_program.StepProgram) the launches that take the newest token of every hypothesis row (bs.tok[:, counter], bs:
        functional.BeamStepState) through the LM, and returns the buffer of the fp32 logits [rows, V_lm].  `state`: init_decode(rows,
        Tmax, anc=the decoder's ancestry table).  Position = the int32 device scalar bs.counter: the embedding reads position
        counter + padding_idx + 1, the layers are step_program.append_layers without encoder attention over state.anc."""
        dec = self.decoder
        rows, Tmax = state.rows, state.Tmax
        if bs.rows != rows or bs.Tmax != Tmax:
            raise ValueError(f"device_step: a decode state of {rows} rows x {Tmax} positions beside a beam state of {bs.rows} x {bs.Tmax}")
        table = dec.embed_tokens.weight.detach()
        pos = dec.embed_positions.table(Tmax + dec.padding_idx + 2, table.device)
        x = prog.new(rows, self.num_heads * self.head_dim)
        prog.add(lambda: Fn.beam_embed_step(table, bs, pos, dec.padding_idx + 1, dec.embed_scale, x))

        def self_attn(q, slots, ctx, H, hd):
            Fn.lm_decode_attn_dev(q, slots, state.anc, bs.counter, 1, Tmax, H, hd, ctx, state.ws)

        y = append_layers(prog, x, list(dec.layers), state.kv, Tmax, bs.counter, self_attn, final_norm=dec.layer_norm)
        proj = dec.output_projection
        return prog.lin(y, [proj.weight], [None], prog.new(rows, proj.weight.shape[0], dt=torch.float32), out_f32=True)

    @torch.no_grad()
    def device_step_sents(self, state, bs, prog):
        """device_step PER SENTENCE SLOT, the LM's share of one step of a beam-search stream (beam_stream.BeamStreamDecode): `bs` is a
        functional.BeamStreamState, every slot of `beam` rows has its own position bs.pos[slot].  The embedding is st5_beam_embed_sents
        with the LM's tables at position pos[slot] + padding_idx + 1, the layers are append_layers(per_row=True) over bs.pos_rows (row
        r's K|V go to slot pos_rows[r] of its cache), the self-attention is st5_lm_decode_attn_rows over state.anc and bs.pos_rows;
        then the final LayerNorm and the output projection with fp32 output.  Returns the buffer of the logits [rows, V_lm].
        `state`: init_decode(rows, cap + 2, anc=bs.anc).  The LM reads the stream's ONE ancestry table, which st5_beam_sents_admit
        resets and st5_beam_reorder_sents reorders: it has no table and no reorder of its own, and an admission does nothing for it.
        A slot handed to a new sentence keeps the K|V of its earlier occupant in the LM's caches.  That is harmless: the admission
        resets the slot's rows of the ancestry table to themselves and its position to 0; the step at position p writes slot p of
        every row of the sentence before the attention of that step reads positions 0 .. p, and a reorder only ever points a row at
        rows of its own sentence slot.  So every (row, position) an attention reads has been written by this sentence, at a step
        <= the current one, and positions behind p are never read."""
        dec = self.decoder
        rows, Tmax = state.rows, state.Tmax
        if bs.rows != rows or bs.Tmax != Tmax:
            raise ValueError(f"device_step_sents: a decode state of {rows} rows x {Tmax} positions beside a stream state of {bs.rows} x "
                             f"{bs.Tmax}")
        if state.anc.data_ptr() != bs.anc.data_ptr():
            raise ValueError("device_step_sents: the decode state must read the stream's ancestry table (init_decode(anc=bs.anc))")
        table = dec.embed_tokens.weight.detach()
        pos = dec.embed_positions.table(Tmax + dec.padding_idx + 2, table.device)
        x = prog.new(rows, self.num_heads * self.head_dim)
        prog.add(lambda: Fn.beam_embed_sents(table, bs, pos, dec.padding_idx + 1, dec.embed_scale, x))

        def self_attn(q, slots, ctx, H, hd):
            Fn.lm_decode_attn_rows(q, slots, state.anc, bs.pos_rows, 1, Tmax, H, hd, ctx, state.ws)

        y = append_layers(prog, x, list(dec.layers), state.kv, Tmax, bs.pos_rows, self_attn, final_norm=dec.layer_norm, per_row=True)
        proj = dec.output_projection
        return prog.lin(y, [proj.weight], [None], prog.new(rows, proj.weight.shape[0], dt=torch.float32), out_f32=True)

    @torch.no_grad()
    def reorder(self, state, order):
        """Row r continues the hypothesis of row order[r] (a beam reorder; len(order) < rows when sentences left the batch)."""
        other = state.bufs[1 - state.cur]
        state.anc = Fn.lm_reorder(state.anc, order, state.t, other)
        state.cur = 1 - state.cur
        return state


def is_fairseq_lm(module):
    """A module with the fairseq `transformer_lm` state-dict layout (what fairseq-generate loads for --lm-path)."""
    if not isinstance(module, nn.Module) or isinstance(module, TransformerLanguageModel):
        return False
    keys = module.state_dict().keys()
    return "decoder.embed_tokens.weight" in keys and not any(k.startswith("encoder.") for k in keys) and \
        any(k.startswith("decoder.layers.") or k.startswith("decoder.adaptive_softmax.") for k in keys)


def convert_fairseq_lm(module, pad=1):
    """TransformerLanguageModel with the weights of a fairseq `transformer_lm` module; the head count and options come from its
    `args` (or its decoder's), else from the first layer's attention module, else the transformer_lm_t5 preset."""
    args = getattr(module, "args", None) or getattr(getattr(module, "decoder", None), "args", None)
    args = Namespace(**vars(args)) if args is not None else Namespace()
    if getattr(args, "decoder_attention_heads", None) is None:
        try:
            args.decoder_attention_heads = int(module.decoder.layers[0].self_attn.num_heads)
        except (AttributeError, IndexError, TypeError):
            pass
    check_supported(_lm_args(args))
    sd = {k: v.detach() for k, v in module.state_dict().items()}
    return TransformerLanguageModel.from_state_dict(sd, args, pad=pad)
