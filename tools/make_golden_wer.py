"""Generates tests/golden/s2t_wer.pt: the validation error counts (c_errors, c_total, w_errors, wv_errors, w_total) that the VERBATIM
reference criterion (SpeechT5/speecht5/criterions/speech_to_text_loss.py, its eval-mode block :232-297) logs for fixed CTC posteriors.

TEST INFRASTRUCTURE ONLY: runs where the reference tree is (imports oracle/ref_stubs.py read-only); the tests read only the fixture it
writes -- recorded inputs and results, no program text.

    python tools/make_golden_wer.py

The criterion runs with ce_weight = 0, ctc_weight = 1 on a stub model in eval mode whose `get_normalized_probs_for_ctc` returns the
case's posterior.  Two names the block needs are not in the reference tree: `editdistance` (third party, absent here; its `eval` is
restated below as the textbook unit-cost Levenshtein distance) and fairseq's `post_process` (speecht5_amd/task.py restates it; the
oracle's identity stub is replaced by it).  The dictionary is speecht5_amd/task.py's `_Dictionary` (fairseq's layout and `string()`).

Cases (modes letter, sentencepiece, None): per-frame argmax paths written out by hand, with an all-blank row, a row of input length 0,
a prediction that collapses to nothing, eos / pad / bos / unk among the argmaxes, leading / doubled / trailing separators, exact ties
(equal maxima: the lowest index wins), a NaN frame, repeated units with and without a blank between them, targets with pad and eos in
the middle, an empty target, and `target` differing from `target_label` (the counts read the latter)."""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_stubs  # noqa: E402
from speecht5_amd.task import _Dictionary, post_process  # noqa: E402

EXTRA = ["<mask>", "<ctc_blank>"]
BOS, PAD, EOS, UNK = 0, 1, 2, 3


def levenshtein(a, b):
    a, b = list(a), list(b)
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (x != y))
    return row[-1]


class StubModel:
    training = False

    def __init__(self, lprobs, lengths):
        self.lprobs = lprobs
        T, B, _ = lprobs.shape
        self.mask = torch.arange(T)[None, :] >= torch.as_tensor(lengths)[:, None]

    def __call__(self, **net_input):
        return None, {"encoder_padding_mask": [self.mask]}

    def get_normalized_probs_for_ctc(self, net_output, log_probs=True):
        return self.lprobs


def posterior(paths, V, seed, ties=(), nans=()):
    """[T, B, V] log-probabilities whose argmax follows paths[b][t]; ties: (b, t, other) gives class `other` the maximum's exact
    value too; nans: (b, t, v) puts a NaN there (it wins the argmax)."""
    g = torch.Generator().manual_seed(seed)
    B, T = len(paths), max(len(p) for p in paths)
    logits = torch.randn(T, B, V, generator=g) * 0.3
    for b, p in enumerate(paths):
        for t, c in enumerate(p):
            logits[t, b, c] += 4.0
    for b, t, other in ties:
        logits[t, b, other] = logits[t, b, paths[b][t]]
    lp = torch.log_softmax(logits, -1)
    for b, t, other in ties:
        assert lp[t, b, other] == lp[t, b, paths[b][t]]
    for b, t, v in nans:
        lp[t, b, v] = float("nan")
    return lp


def pad_rows(rows, fill):
    L = max(len(r) for r in rows)
    return torch.tensor([list(r) + [fill] * (L - len(r)) for r in rows], dtype=torch.long)


def letter_case():
    syms = list("abcde") + ["|", "'"]
    d = _Dictionary(syms, EXTRA)
    ix = {s: d.index(s) for s in syms}
    a, b, c, e, bar, ap = ix["a"], ix["b"], ix["c"], ix["e"], ix["|"], ix["'"]
    bl = d.index("<ctc_blank>")
    paths = [
        [bar, bar, a, b, bl, b, bar, bar, c, c, bar, bar],          # leading / doubled / trailing separators, b blank b = two units
        [bl] * 12,                                                  # all blank
        [a, b, c, bar, a, b, c, bar, a, b, c, bar],                 # input length 0: none of it is read
        [a, EOS, b, PAD, bar, UNK, BOS, c, EOS, EOS, bar, e],       # specials among the argmaxes
        [a, a, a, bl, a, ap, ap, bar, bl, bar, e, e],               # repeats; separator, blank, separator
        [bl, bl, c, bl, bl, bl, bl, bl, bl, bl, bl, bl],            # read for 2 frames only: collapses to nothing
        [a, b, bar, c, e, bar, a, b, bar, c, e, bl],                # two tokenisations meet the same target words
    ]
    lengths = [12, 12, 0, 12, 12, 2, 11]
    labels = [
        [a, b, b, bar, c, EOS],
        [a, bar, b, EOS],
        [c, EOS],
        [a, b, PAD, bar, EOS, c, bar, e, EOS, PAD],                 # pad and eos in the middle
        [a, ap, bar, e, EOS],
        [EOS],                                                      # empty target
        [a, b, bar, c, e, bar, a, b, bar, e, c, EOS],
    ]
    ties = [(4, 0, BOS), (4, 5, a), (0, 8, e)]      # the lower index wins: bos over a; a over '; c over e stays c
    return dict(mode="letter", symbols=syms, paths=paths, lengths=lengths, labels=labels, ties=ties, nans=[(6, 3, a)], seed=1)


def sentencepiece_case():
    us = "▁"
    syms = [us + "the", us, "a", us + "c", "he", "t", us + "ca", "at", "é"]
    d = _Dictionary(syms, EXTRA)
    i = {s: d.index(s) for s in syms}
    bl = d.index("<ctc_blank>")
    paths = [
        [i[us + "the"], bl, i[us + "c"], i["at"], i["at"], bl, i[us], i[us]],           # "the cat" then a trailing lone separator
        [i[us], i["t"], i["he"], i[us + "ca"], i["t"], bl, bl, bl],                     # "the cat" tokenised differently
        [i["a"], i["a"], bl, i["a"], UNK, i[us], i["é"], EOS],                          # "aa<unk> é"
        [bl, bl, bl, bl, bl, bl, bl, bl],
    ]
    lengths = [8, 8, 8, 5]
    labels = [
        [i[us + "the"], i[us + "ca"], i["t"], EOS],
        [i[us + "the"], i[us + "c"], i["at"], EOS],
        [i[us], i["a"], i["a"], i[us], i["é"], EOS, PAD, PAD],
        [i[us + "the"], EOS],
    ]
    return dict(mode="sentencepiece", symbols=syms, paths=paths, lengths=lengths, labels=labels, ties=[(1, 2, bl)], nans=[], seed=2)


def none_case():
    syms = ["ab", "c", "a", "b", "d e", "hello"]
    d = _Dictionary(syms, EXTRA)
    i = {s: d.index(s) for s in syms}
    bl = d.index("<ctc_blank>")
    paths = [
        [i["ab"], i["c"], bl, i["c"], i["hello"], i["hello"]],      # every unit is a word
        [i["a"], i["b"], i["d e"], bl, EOS, UNK],                   # a symbol holding a space is two words
        [bl, i["hello"], bl, bl, bl, bl],
    ]
    lengths = [6, 6, 9]          # above T: the reference's slice clamps it
    labels = [
        [i["ab"], i["c"], i["hello"], EOS],
        [i["ab"], i["d e"], UNK, EOS],
        [i["hello"], i["hello"], EOS, PAD],
    ]
    return dict(mode=None, symbols=syms, paths=paths, lengths=lengths, labels=labels, ties=[], nans=[], seed=3)


def main():
    crit = ref_stubs.load_reference_criterions()
    ed = types.ModuleType("editdistance")
    ed.eval = levenshtein
    sys.modules["editdistance"] = ed
    crit.s2t.post_process = post_process
    out = dict(extra=EXTRA, cases=[])
    for case in (letter_case(), sentencepiece_case(), none_case()):
        d = _Dictionary(case["symbols"], EXTRA)
        task = types.SimpleNamespace(target_dictionary=d, blank_symbol="<ctc_blank>")
        lp = posterior(case["paths"], len(d), case["seed"], case["ties"], case["nans"])
        B = lp.size(1)
        label = pad_rows(case["labels"], PAD)
        # `target` feeds the CTC loss only (one unit + eos per sentence); the counts read target_label
        target = torch.tensor([[d.index(case["symbols"][0]), EOS]] * B)
        sample = dict(net_input={}, target=target, target_label=label, target_lengths=torch.full((B,), 2), ntokens=2 * B)
        cfg = crit.s2t.SpeechtoTextLossConfig()
        cfg.zero_infinity, cfg.post_process, cfg.wer_args, cfg.wer_kenlm_model = True, case["mode"], None, None
        c = crit.s2t.SpeechtoTextLoss(cfg, task, sentence_avg=False, label_smoothing=0.1, ce_weight=0.0, ctc_weight=1.0)
        model = StubModel(lp, [min(n, lp.size(0)) for n in case["lengths"]])
        _, _, log = c(model, sample)
        counts = {k: int(log[k]) for k in ("c_errors", "c_total", "w_errors", "wv_errors", "w_total")}
        # per-sentence counts: the same call on one-sentence batches
        rows = []
        for b in range(B):
            s1 = dict(net_input={}, target=target[b:b + 1], target_label=label[b:b + 1], target_lengths=torch.full((1,), 2), ntokens=2)
            m1 = StubModel(lp[:, b:b + 1].contiguous(), [min(case["lengths"][b], lp.size(0))])
            _, _, l1 = c(m1, s1)
            rows.append([int(l1[k]) for k in ("c_errors", "c_total", "w_errors", "w_total")])
        assert [sum(r[j] for r in rows) for j in range(4)] == [counts["c_errors"], counts["c_total"], counts["w_errors"], counts["w_total"]]
        out["cases"].append(dict(mode=case["mode"], symbols=case["symbols"], lprobs=lp, input_lengths=torch.tensor(case["lengths"]),
                                 target_label=label, blank=d.index("<ctc_blank>"), counts=counts, rows=rows))
        print(case["mode"], counts, rows)
    path = os.path.join(ROOT, "tests", "golden", "s2t_wer.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
