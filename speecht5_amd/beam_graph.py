"""ASR beam search with the step index on the device (SequenceGenerator(decode="device")) and replayed from a HIP graph
(decode="graph"); the mechanism (step program, layer sequence, replay loop) is step_program.py.

The step: the text decoder pre-net's newest row (st5_beam_embed_step), the decoder layers over the slot state (cross-attention:
st5_beam_cross_attn over the sentence-shared K|V), the optional final LayerNorm, the tied output projection with fp32 output, the beam
step (st5_beam_step: log-softmax, rules, candidates, EOS logic, finalisation into per-sentence records, the next tokens; it advances
the counter) and the in-place ancestry reorder (st5_beam_reorder_dev).  Finished sentences are NOT removed from the batch: their rows
keep running and their records are frozen.  Every buffer the graph has baked in belongs to the BeamDeviceDecode object, which
outlives the graph.

The position of the newest token is a function of the step alone, counter + padding_idx + 1: without forced prefixes no hypothesis
contains `pad` (its log-probability is -inf at every step; `prefix_tokens` is refused), which is what SinusoidalPositionalEmbedding
counts.

Joint CTC / attention scoring (ctc_weight > 0) runs in these modes with ctc_rows=True only: no sentence leaves the batch, so row r is
scored against sentence r // beam's own posterior and frame count for the whole call.  The step then is: pre-net row, decoder layers,
projection, st5_beam_ctc_candidates (log-probabilities and the 7 x beam best tokens of every row), st5_ctc_prefix_score_rows_dev (the
rows scorer with out_len and the last labels read on the device, the mix (1 - w) lp + w (log psi - prev) in its epilogue), [the LM
term, see below], st5_beam_step_logprobs (the beam step on log-probabilities), st5_ctc_select_dev (the continued rows' prefix states),
the reorder (csrc/beam_ctc.hip; buffers: functional.BeamCtcState).  A hypothesis continued by a token outside its CTC candidates sets
a sticky device flag (rows that are ignored or belong to a finished sentence do not); the host reads it where it reads the
finished-sentence count and at the end, and raises _generate's KeyError then, a few steps later than the slots loop would.

Shallow fusion (lm_model) runs in these modes when the LM is a speecht5_amd.transformer_lm.TransformerLanguageModel
(task.build_generator converts fairseq LMs to it).  No sentence leaves the batch, so the LM's rows are the decoder's rows with the same
ancestry: the LM's slot caches are read through the DECODER's ancestry table (st.bufs[0]; TransformerLanguageModel.init_decode(anc=)),
there is no second table and no reorder of the LM's own.  Its launches (TransformerLanguageModel.device_step: st5_beam_embed_step with
the LM's tables, the layers on the skinny-M kernel, K|V into slot `counter`, st5_lm_decode_attn_dev, the final LayerNorm, the output
projection with fp32 output) follow the decoder's projection; then st5_beam_lm_logprobs (csrc/beam_lm.hip) puts the LM term into the
step's log-probabilities.  Without CTC: st5_beam_lm_logprobs on the decoder's logits (log-softmax with the beam step's statistics, then
lp[:, :V_lm] += lm_weight * log_softmax(lm logits)), st5_beam_step_logprobs, the reorder.  With CTC: candidates, prefix scores and mix,
st5_beam_lm_logprobs in place on the mixed log-probabilities, st5_beam_step_logprobs, select, the reorder -- _generate's order (CTC
candidates and mix on the unfused log-probabilities, then the LM, then the rules).  The step stays serial.  Without an LM the launch
list is what it is without this paragraph.  Refused, each with a ValueError that names lm_model: any other LM object (the full-prefix
fallback has no device form), an LM with a larger dictionary than the model's (V_lm > vocab_size), and max_len + 2 positions more than
lm.max_positions() (asked at generate(), where max_len is known).

`attention` of the returned hypotheses is an empty tensor in these modes: no probability record is kept."""
import torch

from . import functional as Fn
from .step_program import StepProgram, append_layers, on_decode_stream, run_steps

DECODE_MODES = ("device", "graph")


def check_generator(gen):
    """ValueError naming the option of SequenceGenerator `gen` that the device-stepped modes do not cover (asked at construction)."""
    mode = gen.decode
    if gen.model.models_size != 1:
        raise ValueError(f"decode={mode!r}: more than one model ({gen.model.models_size}) is not supported; use decode='slots'")
    if gen.ctc_weight > 0 and not gen.ctc_rows:
        raise ValueError(f"decode={mode!r}: ctc_weight > 0 needs ctc_rows=True (no sentence leaves the batch here, so every sentence is "
                         f"scored against its own CTC posterior); the first-sentence scoring of ctc_rows=False is decode='slots' only")
    if gen.lm_model is not None:
        from .transformer_lm import TransformerLanguageModel
        lm = gen.lm_model
        if not isinstance(lm, TransformerLanguageModel):
            raise ValueError(f"decode={mode!r}: an LM (lm_model) of type {type(lm).__name__} is not supported (only "
                             f"speecht5_amd.transformer_lm.TransformerLanguageModel has a device-stepped form); use decode='slots'")
        V_lm = lm.decoder.embed_tokens.num_embeddings
        if V_lm > gen.vocab_size:
            raise ValueError(f"decode={mode!r}: lm_model has a dictionary of {V_lm} symbols, more than the model's {gen.vocab_size}")
    if gen.repeat_ngram_blocker is not None:
        raise ValueError(f"decode={mode!r}: no_repeat_ngram_size > 0 is not supported; use decode='slots'")
    if gen.match_source_len:
        raise ValueError(f"decode={mode!r}: match_source_len is not supported; use decode='slots'")
    if gen.custom_search:
        raise ValueError(f"decode={mode!r}: a custom search_strategy is not supported (the device beam step is fairseq's BeamSearch)")
    m = gen.model.models[0]
    dec = getattr(m, "decoder", None)
    if not hasattr(dec, "init_beam_slots") or not hasattr(m, "text_decoder_prenet") or not hasattr(m, "text_decoder_postnet"):
        raise ValueError(f"decode={mode!r} needs a SpeechT5 text decoder with a slot API; {type(m).__name__} has none")
    dec.check_beam_slots()
    if any(l.encoder_attn is None for l in dec.layers):
        raise ValueError(f"decode={mode!r}: a decoder layer has no encoder attention")
    Fn.beam_step_check(gen.beam_size, gen.vocab_size)


def check_lm_positions(gen, max_len):
    """ValueError when the call's max_len + 2 positions are more than the LM takes (asked at generate(): max_len depends on the input)."""
    if gen.lm_model is not None and max_len + 2 > gen.lm_model.max_positions():
        raise ValueError(f"decode={gen.decode!r}: lm_model takes {gen.lm_model.max_positions()} positions, this call needs max_len + 2 = "
                         f"{max_len + 2}; lower max_len_a / max_len_b or use decode='slots'")


def never_mask(gen, device):
    """uint8 [V]: the symbols no hypothesis may contain (SequenceGenerator._never), built once per call."""
    never = torch.zeros(gen.vocab_size, dtype=torch.uint8)
    never[gen.blank] = 1
    if gen.mask != gen.unk:
        never[gen.mask] = 1
    if gen.mask_idxs.numel():
        never[gen.mask_idxs] = 1
    return never.to(device)


class BeamDeviceDecode:
    """Buffers and launch sequence of one generate() call's decode steps."""

    def __init__(self, gen, model, encoder_out, n_sent, max_len, bos):
        beam, V = gen.beam_size, gen.vocab_size
        dec, pre, post = model.decoder, model.text_decoder_prenet, model.text_decoder_postnet
        st = dec.init_beam_slots(n_sent, beam, max_len + 2, encoder_out)
        if st.xkv is None:
            raise ValueError("device-stepped beam search needs an encoder output and decoder layers with an encoder attention")
        dev, dtype = st.bufs[0].device, Fn.compute_dtype()
        rows, C = st.rows, pre.embed_dim
        self.slots, self.gen, self.n_sent, self.max_len = st, gen, n_sent, max_len
        self.bs = Fn.BeamStepState(n_sent, beam, max_len, bos, dev, anc=st.bufs[0])
        bs = self.bs
        self.never = never_mask(gen, dev)
        self.len_div = Fn.beam_len_div(max_len, gen.len_penalty, dev) if gen.normalize_scores else None
        self.host = torch.zeros(2, dtype=torch.int32, pin_memory=True)     # (n_finished, the CTC scorer's `unknown` flag)
        self.ctc = self._ctc_state(gen, model, encoder_out, n_sent, dev) if gen.ctc_weight > 0 else None
        self.event = torch.cuda.Event()
        prog = self.prog = StepProgram(dev, dtype, rows)
        new, lin, add = prog.new, prog.lin, prog.add
        # pre-net: embed_scale * E[token] + pos[counter + padding_idx + 1] (see the module docstring for why the step decides it)
        table = pre.embed_tokens.weight.detach()
        pos = pre.embed_positions.table(max_len + 2 + pre.padding_idx + 2, dev)
        x = new(rows, C)
        add(lambda x=x: Fn.beam_embed_step(table, bs, pos, pre.padding_idx + 1, pre.embed_scale, x))
        layers = list(dec.layers)

        def self_attn(q, slots, ctx, H, hd):      # positions 0 .. counter over st.bufs[0], the one ancestry table, reordered in place
            Fn.lm_decode_attn_dev(q, slots, st.bufs[0], bs.counter, 1, st.Tmax, H, hd, ctx, st.self_ws)

        def cross_attn(idx, q, ctx):              # no step dependence: nothing is recorded
            ca, (kv, k_off) = layers[idx].encoder_attn, st.xkv[idx]
            Fn.beam_cross_attn(q, kv, k_off, st.sent, st.n_sent, st.beam, st.S, ca.num_heads, ca.head_dim, kpm=st.kpm, ws=st.cross_ws,
                               ctx=ctx)

        x = append_layers(prog, x, layers, st.kv, st.Tmax, bs.counter, self_attn, cross_attn, dec.layer_norm)
        # tied output projection, fp32 out (no cast kernel), then the beam step and the ancestry reorder
        proj = post.output_projection
        self.logits = lin(x, [proj.weight], [proj.bias], new(rows, V, dt=torch.float32), out_f32=True)
        rules = dict(temperature=gen.temperature, pad=gen.pad, unk=gen.unk, eos=gen.eos, unk_penalty=gen.unk_penalty, min_len=gen.min_len)
        # shallow fusion: the LM's step over the same rows and the decoder's ancestry table, behind the decoder's projection
        lm, w_lm = gen.lm_model, float(gen.lm_weight)
        self.lm_state = self.lm_logits = self.lp = None
        if lm is not None:
            self.lm_state = lm.init_decode(rows, max_len + 2, anc=st.bufs[0])
            self.lm_logits = lm.device_step(self.lm_state, bs, prog)
        if self.ctc is None and lm is None:
            add(lambda: Fn.beam_step(self.logits, V, bs, self.never, self.len_div, **rules))
        elif self.ctc is None:
            # log-probabilities with the LM term, the beam step on them
            self.lp = new(rows, V, dt=torch.float32)
            add(lambda: Fn.beam_lm_logprobs(self.lp, V, bs, self.lm_logits, w_lm, logits=self.logits, temperature=gen.temperature))
            add(lambda: Fn.beam_step(self.lp, V, bs, self.never, self.len_div, logprobs=True, **rules))
        else:
            # log-probabilities and candidates, prefix scores mixed into them, the LM term, the beam step on them, the continued rows'
            # prefix states
            ctc = self.ctc
            add(lambda: Fn.beam_ctc_candidates(self.logits, V, bs, ctc, self.never, gen.temperature))
            add(lambda: Fn.ctc_prefix_score_rows_dev(bs, ctc))
            if lm is not None:
                add(lambda: Fn.beam_lm_logprobs(ctc.lp, V, bs, self.lm_logits, w_lm))
            add(lambda: Fn.beam_step(ctc.lp, V, bs, self.never, self.len_div, logprobs=True, **rules))
            add(lambda: Fn.ctc_select_dev(bs, ctc))
        add(lambda: Fn.beam_reorder_dev(bs))
        prog.finish()

    def _ctc_state(self, gen, model, encoder_out, n_sent, dev):
        """The CTC posterior and frame counts as _generate builds them for ctc_rows, and the step's CTC buffers."""
        from .sequence_generator import CTC_SCORING_RATIO, CTCPrefixScorerRows
        post = model.get_normalized_probs_for_ctc(encoder_out, log_probs=True).transpose(0, 1)      # B x T x V
        nc = min(post.shape[-1] - gen.mask_idxs.numel(), int(gen.beam_size * CTC_SCORING_RATIO))
        pm = encoder_out["encoder_padding_mask"]
        pm = pm[0] if isinstance(pm, (list, tuple)) and len(pm) > 0 else (pm if isinstance(pm, torch.Tensor) else None)
        frames = torch.full((n_sent,), post.size(1), dtype=torch.int32, device=dev) if pm is None or pm.numel() == 0 \
            else (post.size(1) - pm.sum(dim=1)).to(torch.int32)
        self.ctc_beam = nc
        return Fn.BeamCtcState(CTCPrefixScorerRows(post, frames, gen.blank, gen.eos), self.bs, nc, gen.ctc_weight)

    def buffer_ptrs(self):
        """Data pointers of what must never move during a call: slot K/V, encoder-side K|V, the hypothesis records, the CTC buffers,
        the LM's slot caches, its logits and (without CTC) the fused log-probabilities."""
        st = self.slots
        ctc = () if self.ctc is None else tuple(t.data_ptr() for t in self.ctc.buffers())
        lm = () if self.lm_state is None else tuple(t.data_ptr() for t in self.lm_state.kv) + tuple(
            t.data_ptr() for t in (self.lm_logits, self.lp) if t is not None)
        return tuple(t.data_ptr() for t in st.kv) + tuple(kv.data_ptr() for kv, _ in st.xkv) + (self.bs.records.data_ptr(),
                                                                                                  st.bufs[0].data_ptr()) + ctc + lm

    def poll(self):
        """Sentences finished after the steps enqueued so far: one pinned non-blocking copy (with CTC a second one, of the scorer's
        `unknown` flag) and an event.  KeyError, _generate's, when a hypothesis was continued outside its CTC candidates."""
        self.host[:1].copy_(self.bs.n_finished, non_blocking=True)
        if self.ctc is not None:
            self.host[1:].copy_(self.ctc.unknown, non_blocking=True)
        self.event.record()
        self.event.synchronize()
        if int(self.host[1]):
            raise KeyError("a hypothesis was extended by a token outside its CTC candidate list "
                           f"(ctc_beam={self.ctc_beam}); its prefix state does not exist")
        return int(self.host[0])

    def finalized(self):
        """generate()'s return value from ONE device-to-host read of the records: per sentence the hypotheses best first."""
        bs, beam = self.bs, self.bs.beam
        _, _, score, length, n_hyp, _ = bs.unpack_records(bs.records.cpu())
        out = []
        for s in range(self.n_sent):
            hyps = []
            for k in range(int(n_hyp[s])):
                h = s * beam + k
                n = int(length[h])
                hyps.append({"tokens": bs.rec_tok[h, :n].to(torch.int64), "score": bs.rec_score[h].clone(),
                             "attention": torch.empty(0), "alignment": torch.empty(0), "positional_scores": bs.rec_pos[h, :n].clone()})
            order = torch.sort(score[s * beam: s * beam + len(hyps)], descending=True)[1]
            out.append([hyps[i] for i in order])
        return out


def generate(gen, sample, prefix_tokens=None, constraints=None, bos_token=None):
    """SequenceGenerator._generate in "device" / "graph" mode."""
    mode = gen.decode
    assert mode in DECODE_MODES
    if prefix_tokens is not None:
        raise ValueError(f"decode={mode!r}: prefix_tokens are not supported (the newest position would depend on the prefix's pads); "
                         f"use decode='slots'")
    if constraints is not None:
        raise ValueError(f"decode={mode!r}: constraints are not supported")
    check_generator(gen)          # (the generator's attributes may have changed since construction)
    net_input = sample["net_input"]
    src_tokens, _ = gen._source_lengths(net_input)
    n_sent, src_len = src_tokens.size()[:2]
    max_len = min(int(gen.max_len_a * src_len + gen.max_len_b), gen.max_len - 1)
    assert gen.min_len <= max_len, "min_len cannot be larger than max_len, please adjust these!"
    check_lm_positions(gen, max_len)
    model = gen.model.models[0]
    encoder_outs = gen.model.forward_encoder(net_input, exact_rows=True) if gen.exact_rows else gen.model.forward_encoder(net_input)
    stats = {"polls": 0, "device_steps": 0, "graph_replays": 0}
    with on_decode_stream(model, src_tokens.device, mode) as caller:
        st = BeamDeviceDecode(gen, model, encoder_outs[0], n_sent, max_len, gen.eos if bos_token is None else bos_token)
        first = st.buffer_ptrs()
        # steps 0 .. max_len.  When the schedule runs out, the steps behind the last poll may have set the CTC scorer's `unknown` flag
        # (the last group never polls: step max_len finishes every sentence): read it once more.  Not an extra synchronisation of every
        # call (a call that ends at a poll does not get here; finalized() synchronises next anyway), and not counted in stats["polls"],
        # which counts the schedule's polls.
        if not run_steps(st.prog.step, max_len + 1, mode, gen.BEAM_POLL_STEPS, lambda: st.poll() == n_sent, stats) and st.ctc is not None:
            st.poll()
        out = st.finalized()
        last = st.buffer_ptrs()
    if caller is not None:
        for hyps in out:
            for h in hyps:
                for t in (h["tokens"], h["score"], h["positional_scores"]):
                    t.record_stream(caller)
    gen.beam_decode_mode = mode
    gen.beam_polls, gen.beam_device_steps, gen.beam_graph_replays = stats["polls"], stats["device_steps"], stats["graph_replays"]
    gen.beam_buffer_ptrs = (first, last)
    return out
