"""Generates tests/golden/tiny_s2s.pt: speech-to-speech fine-tuning (t5_task s2s: voice conversion, and speech enhancement through
--se-predict / --se-decoder-input) cases of the VERBATIM reference model (SpeechT5/speecht5/models/speecht5.py), its SpeechT5Criterion
(criterions/speecht5_criterion.py -> text_to_speech_loss.py) and its SpeechToSpeechDataset.collater (data/speech_to_speech_dataset.py).

TEST INFRASTRUCTURE ONLY: runs where the reference tree is (imports oracle/ref_stubs.py, oracle/make_golden.py,
oracle/make_golden_collate2.py and oracle/make_golden_metrics.py read-only); the tests read only the fixture it writes.

    python tools/make_golden_s2s.py

Model: the shared tiny trunk (tests/golden/tiny_model.pt, weights taken from there where the shapes agree) under arch
t5_transformer_base_asr with the VC recipe's switches (no codebook, mask probabilities 0) and every dropout 0 -- the decoder pre-net's
always-on dropout included (dprenet_dropout_rate 0, as oracle/make_golden.py has it for tiny_t2s.pt).  Only what tiny_model.pt does
not hold is stored, once per reduction factor (with r = 1: the frame / stop projections and the decoder pre-net's first layer).  B = 3 with ragged source and target lengths;
the batch is the reference collater's own.  With se_decoder_input=source or se_predict the reference reads net_input["src_tokens"] /
["src_lengths"] (the source utterance's features), which its collater does not supply: they are added here, of the length the
decoder output has.

Per case: train-mode outputs of model(**net_input), the SpeechT5Criterion loss / logging output / reduce_metrics calls, gradient norms
of every parameter plus the full gradients of the post-net and of a few trunk tensors, eval-mode outputs, generate_speech(source=...)
on one clip, the state-dict key list after prune_modules("s2s").  Plus batches of the reference collater for the item sets of
COLLATE_SETS at r = 1 and 2."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_stubs  # noqa: E402
import make_golden as mg  # noqa: E402

ODIM, SPK = 80, 64
# full gradients: the whole post-net in the cases of FULL_POSTNET (the file stays under the committed-size limit), its small tensors
# and a few trunk tensors in every case
FULL_POSTNET = ("masking",)
FULL_GRADS = ("speech_decoder_postnet.prob_out.", "speech_decoder_postnet.feat_out.bias", "speech_decoder_postnet.postnet.postnet.4.1.",
              "decoder.layers.1.final_layer_norm.", "encoder.layer_norm.", "decoder.layers.1.encoder_attn.v_proj.bias",
              "encoder.layers.1.final_layer_norm.", "speech_decoder_prenet.decoder_prenet.1.alpha")
LENS = [(2000, 9), (1600, 6), (1100, 5)]      # (source samples, target frames) of the model batch

CASES = dict(
    recipe=dict(r=2, se_decoder_input="previous_target", se_predict=None, guided=True),
    source_in=dict(r=2, se_decoder_input="source", se_predict=None),
    masking=dict(r=1, se_decoder_input="source", se_predict="masking"),
    target=dict(r=1, se_decoder_input="source", se_predict="target"),
    delta=dict(r=1, se_decoder_input="source", se_predict="delta"),
    delta_prev=dict(r=1, se_decoder_input="previous_target", se_predict="delta"),
)

# (source samples, target frames) per item
COLLATE_SETS = dict(
    one=[(350, 9)],
    equal=[(320, 8), (320, 8), (320, 8)],
    odd_target=[(450, 11), (260, 7), (370, 5)],
    one_frame=[(300, 1), (225, 6)],
    single_frame=[(250, 1)],
    longest_first=[(500, 4), (150, 10), (499, 3), (17, 2)],
)


class S2sTask:
    def __init__(self):
        self.dicts = {"text": mg.Dictionary(30, ["<mask>", "<ctc_blank>"])}
        self.t5_task = "s2s"
        self.target_dictionary = self.dicts["text"]
        self.blank_symbol_idx = self.dicts["text"].index("<ctc_blank>")
        self.blank_symbol = "<ctc_blank>"


def s2s_args(case):
    over = dict(reduction_factor=case["r"], se_decoder_input=case["se_decoder_input"])
    if case["se_predict"] is not None:
        over["se_predict"] = case["se_predict"]
    return mg.tiny_args("t5_transformer_base_asr", use_codebook=False, mask_prob=0.0, mask_channel_prob=0.0, relative_position_embedding=True,
                        **over)


def items(spec, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (n, L) in enumerate(spec):
        out.append({"id": 10 + i, "source": torch.randn(n, generator=g), "target": torch.randn(L, ODIM, generator=g) * 0.5 - 1,
                    "spkembs": torch.randn(SPK, generator=g), "audio_name": f"src{i}-tgt{i}.wav", "tgt_name": f"spk/tgt{i}.wav"})
    return out


def dataset(mod, r):
    ds = object.__new__(mod.SpeechToSpeechDataset)
    ds.reduction_factor = r
    return ds


def clone(x, memo=None):
    """Deep copy that keeps one tensor one tensor (the collater's "target" IS its "dec_target": stored once)."""
    memo = {} if memo is None else memo
    if torch.is_tensor(x):
        if id(x) not in memo:
            memo[id(x)] = x.clone()
        return memo[id(x)]
    if isinstance(x, dict):
        return {k: clone(v, memo) for k, v in x.items()}
    if isinstance(x, list):
        return [clone(v, memo) for v in x]
    return x


def sample_for(mod, case, base_items):
    """The reference collater's batch, plus src_tokens / src_lengths where the case's forward reads them."""
    s = dataset(mod, case["r"]).collater(base_items)
    if case["se_decoder_input"] == "source" or case["se_predict"] is not None:
        olens = s["dec_target_lengths"]
        B, Lmax = s["dec_target"].shape[:2]
        Ls = Lmax // case["r"]                       # the decoder then emits Ls * r = the trimmed target length
        g = torch.Generator().manual_seed(33)
        src = torch.randn(B, Ls, ODIM, generator=g) * 0.5 - 1
        lens = torch.div(olens, case["r"], rounding_mode="floor")
        for b in range(B):
            src[b, int(lens[b]):] = 0
        s["net_input"]["src_tokens"], s["net_input"]["src_lengths"] = src, lens
    return s


def grads_record(model, prefixes):
    norms, full = {}, {}
    for n, p in model.named_parameters():
        if p.grad is None:
            continue
        norms[n] = float(p.grad.double().norm())
        if n.startswith(prefixes):
            full[n] = p.grad.detach().clone()
        p.grad = None
    return dict(norms=norms, full=full)


def reduce_calls(crit_mod, log, loss):
    import importlib
    mgm = importlib.import_module("make_golden_metrics")
    rec = mgm.Recorder()
    old = crit_mod.metrics
    crit_mod.metrics = rec
    try:
        crit_mod.SpeechT5Criterion.reduce_metrics([{"loss": loss, "sample_size": 1, "ntokens": log["ntokens"], "s2s": log}])
    finally:
        crit_mod.metrics = old
    return rec.calls


def main():
    import importlib
    ref = ref_stubs.load_reference_models()
    ref_stubs.load_reference_criterions()
    crit_mod = importlib.import_module("speecht5.criterions.speecht5_criterion")
    import make_golden_collate2 as mgc
    mod = mgc.load("speech_to_speech_dataset")
    tiny = torch.load(os.path.join(mg.OUT, "tiny_model.pt"))["state_dict"]
    task = S2sTask()
    base_items = items(LENS, seed=21)
    gen_clip = torch.randn(1, 900, generator=torch.Generator().manual_seed(22))      # (2 encoder frames: generate_speech stops at 20 frames)
    out = dict(samples={r: clone(dataset(mod, r).collater(base_items)) for r in (1, 2)}, gen_clip=gen_clip, state={}, trunk_keys={},
               cases={})
    for name, case in CASES.items():
        args = s2s_args(case)
        model = mg.build(ref, args, "t5_transformer_base_asr", task, seed=40)
        own = model.state_dict()
        trunk = {k: v for k, v in tiny.items() if k in own and own[k].shape == v.shape}
        torch.nn.Module.load_state_dict(model, trunk, strict=False)
        state = {k: v.clone() for k, v in model.state_dict().items() if k not in trunk}
        r = case["r"]
        if r in out["state"]:                      # same seed, same shapes: what the trunk does not hold is the same for every case of one r
            assert state.keys() == out["state"][r].keys() and all(torch.equal(v, out["state"][r][k]) for k, v in state.items())
        out["state"][r], out["trunk_keys"][r] = state, sorted(trunk)
        start = {k: v.clone() for k, v in model.state_dict().items()}
        sample = sample_for(mod, case, base_items)
        c = crit_mod.SpeechT5Criterion(task, False, 0.1, 1.0, 0.0, loss_weights=[0.1], log_keys=[],
                                       use_guided_attn_loss=bool(case.get("guided")))
        model.train()
        torch.manual_seed(3)
        before, after, logits, attn = model(**sample["net_input"])
        train_out = dict(before=before.detach(), after=after.detach(), stop_logits=logits.detach(), attn=[a.detach() for a in attn])
        model.load_state_dict(start)               # (the forward above moved the BatchNorm running statistics)
        torch.manual_seed(3)
        loss, sample_size, log = c(model, sample)
        (loss / sample_size).backward()
        grads = grads_record(model, FULL_GRADS + (("speech_decoder_postnet.",) if name in FULL_POSTNET else ()))
        log = {k: (float(v) if isinstance(v, float) else v) for k, v in log.items() if isinstance(v, (int, float))}
        calls = reduce_calls(crit_mod, log, float(loss) / sample_size)
        model.load_state_dict(start)
        model.eval()
        with torch.no_grad():
            eb, ea, el, eattn = model(**sample["net_input"])
            mel, probs, _ = model.generate_speech(source=gen_clip, padding_mask=torch.zeros(1, gen_clip.shape[1], dtype=torch.bool),
                                                  spkembs=sample["net_input"]["spkembs"][:1])
        model.prune_modules("s2s")
        extra = {k: sample["net_input"][k].clone() for k in ("src_tokens", "src_lengths") if k in sample["net_input"]}
        pruned = list(model.state_dict().keys())
        assert out.setdefault("pruned_keys", pruned) == pruned
        rec = dict(args=dict(vars(args)), case=dict(case), net_input_extra=extra, train=train_out,
                   loss=loss.detach(), sample_size=sample_size, log=log, reduce_calls=calls, grads=grads,
                   eval=dict(after=ea, stop_logits=el), generated_mel=mel, generated_probs=probs)
        out["cases"][name] = rec
        print(f"{name:12s} loss {float(loss):.5f} log {sorted(log)} out {tuple(before.shape)} generated {tuple(mel.shape)} "
              f"stored {sum(v.numel() for v in state.values())} floats, trunk {len(trunk)} of {len(own)} keys")

    out["collate"] = {}
    for si, (sname, spec) in enumerate(COLLATE_SETS.items()):
        its = items(spec, seed=50 + si)
        out["collate"][sname] = dict(items=clone(its), batches={r: clone(dataset(mod, r).collater(its)) for r in (1, 2)})
        print("collate", sname, {k: tuple(v.shape) for k, v in out["collate"][sname]["batches"][2]["net_input"].items() if torch.is_tensor(v)})
    assert dataset(mod, 2).collater([]) == {}
    path = os.path.join(ROOT, "tests", "golden", "tiny_s2s.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    np.random.seed(0)
    torch.manual_seed(0)
    main()
