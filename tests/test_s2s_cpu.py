"""Speech-to-speech fine-tuning (t5_task s2s), host side: the fixture of the verbatim reference (tests/golden/tiny_s2s.pt,
tools/make_golden_s2s.py) is what the GPU tests expect it to be, the GPU collater's host bookkeeping agrees with the reference
collater's recorded batches, and the VC recipe's command line parses."""
import os

import pytest
import torch

from tests.util import G

CASES = {"recipe": (2, "previous_target", None), "source_in": (2, "source", None), "masking": (1, "source", "masking"),
         "target": (1, "source", "target"), "delta": (1, "source", "delta"), "delta_prev": (1, "previous_target", "delta")}
SETS = ["one", "equal", "odd_target", "one_frame", "single_frame", "longest_first"]


@pytest.fixture(scope="module")
def fx():
    return torch.load(os.path.join(G, "tiny_s2s.pt"), weights_only=False)


def test_fixture_cases_shapes_and_keys(fx):
    assert list(fx["cases"]) == list(CASES) and sorted(fx["samples"]) == [1, 2] and list(fx["collate"]) == SETS
    assert os.path.getsize(os.path.join(G, "tiny_s2s.pt")) < (1 << 20)
    tiny = torch.load(os.path.join(G, "tiny_model.pt"), weights_only=False)["state_dict"]
    for name, (r, dec_in, pred) in CASES.items():
        c = fx["cases"][name]
        a = c["args"]
        assert (a["reduction_factor"], a["se_decoder_input"], a.get("se_predict")) == (r, dec_in, pred), name
        assert a["use_codebook"] is False and a["mask_prob"] == 0.0 and a["mask_channel_prob"] == 0.0 and a["dprenet_dropout_rate"] == 0.0
        s = fx["samples"][r]
        B, Lmax, odim = s["dec_target"].shape
        assert (B, odim) == (3, 80) and s["task_name"] == s["net_input"]["task_name"] == "s2s"
        assert len(set(s["src_lengths"].tolist())) == 3 and len(set(s["dec_target_lengths"].tolist())) == 3      # ragged both ways
        L_out = Lmax - Lmax % r
        for k in ("before", "after"):
            assert c["train"][k].shape == (B, L_out, odim), (name, k)
        assert c["train"]["stop_logits"].shape == (B, L_out) and c["eval"]["after"].shape == (B, L_out, odim)
        assert ("src_tokens" in c["net_input_extra"]) == (dec_in == "source" or pred is not None)
        if "src_tokens" in c["net_input_extra"]:
            assert c["net_input_extra"]["src_tokens"].shape == (B, Lmax // r, odim)
        assert ("enc_dec_attn_loss" in c["log"]) == (name == "recipe")
        assert {"loss", "l1_loss", "l2_loss", "bce_loss", "decoder_alpha", "ntokens", "nsentences", "sample_size"} <= set(c["log"])
        assert c["log"]["ntokens"] == int(s["src_lengths"].sum()) and c["sample_size"] == 1
        names = [call[1] for call in c["reduce_calls"]]
        assert names[:5] == ["s2s_loss", "s2s_l1_loss", "s2s_l2_loss", "s2s_bce_loss", "s2s_decoder_alpha"] and names[-1] == "loss"
        assert ("s2s_enc_dec_attn_loss" in names) == (name == "recipe")
        assert set(c["grads"]["full"]) <= set(c["grads"]["norms"]) and len(c["grads"]["norms"]) > 100
        assert c["generated_mel"].shape[1] == odim and c["generated_mel"].shape[0] == c["generated_probs"].shape[0]
        # only what the shared trunk does not hold is stored
        assert set(fx["trunk_keys"][r]) <= set(tiny) and not set(fx["state"][r]) & set(fx["trunk_keys"][r])
    assert fx["state"][2] == {} and all(k.startswith(("speech_decoder_prenet.", "speech_decoder_postnet.")) for k in fx["state"][1])
    assert any(k.startswith("speech_decoder_postnet.postnet.postnet.0.0.") for k in fx["cases"]["masking"]["grads"]["full"])
    pruned = fx["pruned_keys"]
    assert not any(k.startswith(("text_", "speaker_decoder_postnet.", "quantizer.")) for k in pruned)
    assert {k.split(".")[0] for k in pruned} == {"encoder", "decoder", "speech_encoder_prenet", "speech_decoder_prenet", "speech_decoder_postnet"}


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("name", SETS)
def test_collater_bookkeeping_matches_the_recorded_batches(fx, name, r):
    from speecht5_amd.collate import SpeechToSpeechCollater
    col = fx["collate"][name]
    items, ref = col["items"], col["batches"][r]
    audio_sizes, fbank_sizes = [int(it["source"].shape[0]) for it in items], [int(it["target"].shape[0]) for it in items]
    p = SpeechToSpeechCollater.plan(audio_sizes, fbank_sizes, r)
    ni = ref["net_input"]
    assert ni["source"].shape == ni["padding_mask"].shape == (len(items), p["S"])
    assert ref["dec_target"].shape[1] == ref["labels"].shape[1] == p["Lmax"]
    assert ni["prev_output_tokens"].shape[1] == p["Lin"]
    assert ni["tgt_lengths"].tolist() == p["tgt_lengths"] and ref["dec_target_lengths"].tolist() == fbank_sizes
    assert ref["src_lengths"].tolist() == audio_sizes and ref["ntokens"] == p["ntokens"]
    assert ref["name"] == [it["audio_name"] for it in items] and ref["tgt_name"] == [it["tgt_name"] for it in items]
    assert ref["id"].tolist() == [it["id"] for it in items]
    assert ref["target"].data_ptr() == ref["dec_target"].data_ptr()      # one tensor under two keys, in the reference and in the file


def test_empty_sample_list_gives_an_empty_batch():
    from speecht5_amd.collate import SpeechToSpeechCollater
    assert SpeechToSpeechCollater(torch.device("cpu")).collater([]) == {}
    assert SpeechToSpeechCollater(torch.device("cpu")).collater([{"source": None}]) == {}


VC = """DATA --save-dir SAVE --tensorboard-logdir SAVE --train-subset train --valid-subset valid --hubert-label-dir LABELS
 --distributed-world-size 8 --distributed-port 0 --ddp-backend legacy_ddp --user-dir USER --log-format json --seed 1 --fp16
 --task speecht5 --t5-task s2s --sample-rate 16000 --num-workers 4 --max-tokens 1280000 --update-freq 3 --max-tokens-valid 1280000
 --criterion speecht5 --use-guided-attn-loss --report-accuracy --sentence-avg --optimizer adam --dropout 0.2 --activation-dropout 0.2
 --attention-dropout 0.2 --encoder-layerdrop 0.05 --decoder-layerdrop 0.0 --clip-norm 1.0 --lr 0.0001 --lr-scheduler inverse_sqrt
 --warmup-updates 6000 --feature-grad-mult 1.0 --max-update 60000 --max-text-positions 600 --min-speech-sample-size 1056
 --max-speech-sample-size 480256 --max-speech-positions 1876 --required-batch-size-multiple 1 --skip-invalid-size-inputs-valid-test
 --keep-last-epochs 10 --save-interval-updates 10000 --disable-validation --log-interval 10 --arch t5_transformer_base_asr
 --share-input-output-embed --find-unused-parameters --bert-init --relative-position-embedding --mask-prob 0.0 --mask-channel-prob 0.0
 --finetune-from-model CKPT""".split()


def _parse(argv):
    """fairseq's parse_args_and_arch with --user-dir registered, as tests/test_cli_surface.py drives it; the generic fairseq options
    the VC recipe adds to the ASR one (--max-tokens-valid, --disable-validation, --log-interval) and the criterion's
    --use-guided-attn-loss (a TexttoSpeechLoss constructor argument the reference's dataclass does not declare) are declared here."""
    import argparse
    from speecht5_amd import cli
    from speecht5_amd.fairseq_compat import ARCH_REGISTRY, MODEL_REGISTRY, TASK_REGISTRY
    from tests.test_cli_surface import _fairseq_generic
    p = argparse.ArgumentParser(allow_abbrev=False)
    _fairseq_generic(p)
    p.add_argument("--max-tokens-valid", type=int)
    p.add_argument("--log-interval", type=int)
    p.add_argument("--disable-validation", action="store_true")
    p.add_argument("--use-guided-attn-loss", action="store_true")
    pre, _ = p.parse_known_args(argv)
    TASK_REGISTRY[pre.task].add_args(p)
    cli.declare_criterion(p)
    MODEL_REGISTRY["t5_transformer"].add_args(p.add_argument_group("Model-specific configuration", argument_default=argparse.SUPPRESS))
    args = p.parse_args(argv)
    ARCH_REGISTRY[args.arch](args)
    return args


def test_vc_recipe_command_line_parses():
    args = _parse(VC)
    assert args.t5_task == "s2s" and args.max_speech_sample_size == 480256 and args.min_speech_sample_size == 1056
    assert args.mask_prob == 0.0 and args.mask_channel_prob == 0.0 and args.feature_grad_mult == 1.0 and args.encoder_layerdrop == 0.05
    assert args.se_decoder_input == "previous_target" and getattr(args, "se_predict", None) is None and args.reduction_factor == 2
    # the SE variant's switches
    for pred in ("masking", "target", "delta"):
        a = _parse(VC + ["--se-predict", pred, "--se-decoder-input", "source", "--reduction-factor", "1"])
        assert (a.se_predict, a.se_decoder_input, a.reduction_factor) == (pred, "source", 1)
    with pytest.raises(SystemExit):
        _parse(VC + ["--se-predict", "mask"])
