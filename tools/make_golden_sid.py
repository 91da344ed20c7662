"""Generates tests/golden/tiny_s2c.pt: speaker identification (t5_task s2c) cases of the VERBATIM reference model
(SpeechT5/speecht5/models/speecht5.py + models/modules/speaker_decoder_postnet.py), its SpeechtoTextLoss(report_accuracy=True) and
its SpeechToClassDataset.collater.

TEST INFRASTRUCTURE ONLY: runs where the reference tree is (imports oracle/ref_stubs.py, oracle/make_golden.py and
oracle/make_golden_collate2.py read-only); the tests read only the fixture it writes.

    python tools/make_golden_sid.py

Model: the shared tiny trunk (tests/golden/tiny_model.pt, weights taken from there where the shapes agree) under arch
t5_transformer_base_asr with the SID recipe's switches (no codebook, mask probabilities 0, feature_grad_mult 1), and a speaker
dictionary of 15 speakers: class_num = 4 specials + 15 + <mask> + <ctc_blank> = 21 (odd, as the recipe's 1257).  Only what is not
in tiny_model.pt is stored per case (the head, the dictionary-sized embedding).  B = 3 with ragged padding.

Per case: the train-mode loss and logging output, gradient norms of every parameter plus the full gradients of the head and of a few
trunk tensors, BatchNorm running statistics after the step, eval logits and embeds, generate_class output, the state-dict key list."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_stubs  # noqa: E402
import make_golden as mg  # noqa: E402

N_SPK = 15
EMBED = 32
FULL_GRADS = ("speaker_decoder_postnet.", "decoder.layers.1.final_layer_norm.", "encoder.layer_norm.",
              "decoder.layers.1.encoder_attn.v_proj.bias", "encoder.layers.1.final_layer_norm.")

CASES = dict(
    recipe=dict(sid_no_pooling_bn=True, sid_no_embed_postnet=True),
    default=dict(),
    normalize=dict(sid_normalize_postnet=True),
    amsoftmax=dict(sid_softmax_type="amsoftmax", softmax_margin=0.2, softmax_scale=30.0, target_list=True),
    aamsoftmax=dict(sid_no_pooling_bn=True, sid_no_embed_postnet=True, sid_softmax_type="aamsoftmax", softmax_margin=0.2,
                    softmax_scale=30.0, target_list=True, craft=True),
    aamsoftmax_easy=dict(sid_no_pooling_bn=True, sid_no_embed_postnet=True, sid_softmax_type="aamsoftmax", softmax_margin=0.2,
                         softmax_scale=30.0, softmax_easy_margin=True, target_list=True, craft=True),
    encoder=dict(sid_pooling_layer="encoder", sid_no_pooling_bn=True, sid_no_embed_postnet=True),
    encoder_cls=dict(sid_pooling_layer="encoder-cls"),
)


class SidTask:
    def __init__(self):
        self.dicts = {"text": mg.Dictionary(N_SPK, ["<mask>", "<ctc_blank>"])}
        self.t5_task = "s2c"
        self.target_dictionary = self.dicts["text"]
        self.blank_symbol_idx = self.dicts["text"].index("<ctc_blank>")
        self.blank_symbol = "<ctc_blank>"


def sid_args(case):
    over = {k: v for k, v in case.items() if k not in ("target_list", "craft")}
    a = mg.tiny_args("t5_transformer_base_asr", use_codebook=False, mask_prob=0.0, mask_channel_prob=0.0, feature_grad_mult=1.0,
                     relative_position_embedding=True, sid_embed_dim=EMBED, **over)
    return a


def batch(seed=21):
    g = torch.Generator().manual_seed(seed)
    lens = [6000, 4700, 3300]
    S = max(lens)
    src = torch.randn(3, S, generator=g)
    pm = torch.zeros(3, S, dtype=torch.bool)
    for i, n in enumerate(lens):
        src[i, n:] = 0
        pm[i, n:] = True
    target = torch.tensor([[7], [12], [4 + N_SPK - 1]])
    return dict(net_input=dict(source=src, padding_mask=pm, prev_output_tokens=torch.full((3, 1), 2, dtype=torch.long), task_name="s2c"),
                id=torch.arange(3), target=target, target_lengths=torch.ones(3, dtype=torch.long), task_name="s2c", ntokens=3)


def grads_record(model):
    norms, full = {}, {}
    for n, p in model.named_parameters():
        if p.grad is None:
            continue
        norms[n] = float(p.grad.double().norm())
        if n.startswith(FULL_GRADS):
            full[n] = p.grad.detach().clone()
        p.grad = None
    return dict(norms=norms, full=full)


def craft(model, sample):
    """Projection rows for the margin cases: row 0's target cosine below th = cos(pi - m) (about -0.995), row 1's near +0.995, row 2's
    as drawn -- both branches of AdditiveAngularMargin (and both signs for the easy margin)."""
    with torch.no_grad():
        model.train()
        (_, embed), _ = model(**sample["net_input"])
        W = model.speaker_decoder_postnet.output_projection.weight
        g = torch.Generator().manual_seed(5)
        for row, sign in ((0, -1.0), (1, 1.0)):
            e = embed[row] / embed[row].norm()
            noise = torch.randn(e.shape, generator=g)
            noise = noise - (noise @ e) * e
            w = sign * e + 0.1 * noise / noise.norm()
            W[int(sample["target"][row, 0])] = w * W.norm(dim=1).mean() / w.norm()


def main():
    ref = ref_stubs.load_reference_models()
    crit = ref_stubs.load_reference_criterions()
    tiny = torch.load(os.path.join(mg.OUT, "tiny_model.pt"))["state_dict"]
    task = SidTask()
    sample = batch()
    out = dict(n_spk=N_SPK, embed_dim=EMBED, sample=sample, cases={})
    for ci, (name, case) in enumerate(CASES.items()):
        args = sid_args(case)
        model = mg.build(ref, args, "t5_transformer_base_asr", task, seed=40)
        own = model.state_dict()
        trunk = {k: v for k, v in tiny.items() if k in own and own[k].shape == v.shape}
        torch.nn.Module.load_state_dict(model, trunk, strict=False)
        if "shared_state" in out:   # what is neither trunk nor head: the first case's, in every case
            torch.nn.Module.load_state_dict(model, out["shared_state"], strict=False)
        with torch.no_grad():   # BatchNorm affine parameters off their trivial init, so parity is not vacuous
            g = torch.Generator().manual_seed(90 + ci)
            for n, p in model.named_parameters():
                if n.startswith("speaker_decoder_postnet.bn_"):
                    p.add_(torch.randn(p.shape, generator=g) * 0.1)
        s = {k: (dict(v) if isinstance(v, dict) else v) for k, v in sample.items()}
        s["net_input"] = dict(sample["net_input"])
        if case.get("target_list"):
            s["net_input"]["target_list"] = sample["target"]
        if case.get("craft"):
            craft(model, s)
        state = {k: v.clone() for k, v in model.state_dict().items() if k not in trunk or not torch.equal(v, trunk[k])}
        head = {k: v for k, v in state.items() if k.startswith("speaker_decoder_postnet.")}
        rest = {k: v for k, v in state.items() if k not in head}
        if "shared_state" not in out:
            out["shared_state"], out["trunk_keys"] = rest, sorted(trunk)
        assert rest.keys() == out["shared_state"].keys() and all(torch.equal(v, out["shared_state"][k]) for k, v in rest.items())
        assert sorted(trunk) == out["trunk_keys"]
        seen = {}
        hook = model.speaker_decoder_postnet.register_forward_hook(lambda m, i, o: seen.update(logits=o[0].detach().clone()))
        cfgc = crit.s2t.SpeechtoTextLossConfig()
        cfgc.zero_infinity, cfgc.post_process, cfgc.wer_args, cfgc.wer_kenlm_model = True, "letter", None, None
        c = crit.s2t.SpeechtoTextLoss(cfgc, task, sentence_avg=False, label_smoothing=0.1, report_accuracy=True, ce_weight=1.0,
                                      ctc_weight=0.0)
        model.train()
        torch.manual_seed(3)
        loss, sample_size, log = c(model, s)
        (loss / sample_size).backward()
        grads = grads_record(model)
        hook.remove()
        train_logits = seen["logits"]
        bn_state = {k: v.clone() for k, v in model.state_dict().items() if ".bn_" in k}
        model.eval()
        with torch.no_grad():
            (logits, embed), _ = model(**s["net_input"])
            cls = model.generate_class(sample["net_input"]["source"], sample["net_input"]["prev_output_tokens"],
                                       padding_mask=sample["net_input"]["padding_mask"])
        rec = dict(args={k: v for k, v in vars(args).items()}, target_list=bool(case.get("target_list")), state=head, state_keys=list(model.state_dict().keys()), loss=loss.detach(), sample_size=sample_size,
                   log={k: v for k, v in log.items() if isinstance(v, (int, float))}, grads=grads, train_logits=train_logits.detach(),
                   bn_state=bn_state, eval_logits=logits, eval_embed=embed, classes=cls)
        if case.get("craft"):
            W = model.speaker_decoder_postnet.output_projection.weight
            cosv = torch.nn.functional.linear(torch.nn.functional.normalize(embed), torch.nn.functional.normalize(W))
            rec["target_cos"] = cosv.gather(1, sample["target"]).squeeze(1)
            print(f"  target cosines {rec['target_cos'].tolist()} th {math.cos(math.pi - args.softmax_margin):.4f}")
        out["cases"][name] = rec
        print(f"{name:16s} loss {float(loss):.5f} acc {log['n_correct']}/{log['total']} classes {cls.tolist()} "
              f"state {sum(v.numel() for v in state.values())} floats")

    # one batch of the reference SpeechToClassDataset.collater (items cropped by sample_from_feature, numpy's stream)
    import make_golden_collate2 as mgc
    mod = mgc.load("speech_to_class_dataset")
    ds = object.__new__(mod.SpeechToClassDataset)
    ds.tgt_dict = task.dicts["text"]
    np.random.seed(8)
    rng = np.random.RandomState(4)
    items = []
    for i, (n, spk) in enumerate(((900, 5), (520, 11), (740, 9), (300, 17))):
        wav = mod.sample_from_feature(rng.randn(n), 640)
        items.append({"id": i, "source": torch.from_numpy(wav).float(), "label": torch.IntTensor([spk])})
    b = ds.collater(items)
    out["collate"] = dict(items=[{k: (v.clone() if torch.is_tensor(v) else v) for k, v in it.items()} for it in items], batch=b)
    path = os.path.join(ROOT, "tests", "golden", "tiny_s2c.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    np.random.seed(0)
    torch.manual_seed(0)
    main()
