"""Validation UER / WER counts of the ASR criterion (SpeechT5/speecht5/criterions/speech_to_text_loss.py:232-297): per sentence, the
greedy CTC decoding of the encoder's posterior against the target, in units (edit distance of token ids) and in words (edit distance
of `post_process(dictionary.string(tokens), mode).split()`), summed over the batch into c_errors, c_total, w_errors, wv_errors, w_total.

On the GPU the counts come from csrc/asr_metrics.hip (`count_errors`): nothing is copied to the host.  The word split runs on bytes
through a per-symbol table, because for the modes None / "none" / "letter" / "sentencepiece" / "wordpiece" the reference's string form
factors per symbol: with s_i = dictionary[i],

    g(i) = ""                      for bos and eos (Dictionary.string drops them)
    g(i) = "<unk>" for unk, else s_i;  then  g + " "  (None / "none")  or  g.replace(" ", "").replace(SEP, " ")  (SEP = | / U+2581 / _)
    every character with str.isspace() -> one 0x20, the rest UTF-8

and the sentence's words are the non-empty pieces of b"".join(g[t] for t in tokens).split(b" ").  The other modes ("silence", "_EOW",
"subword_nmt", "@@ ", "@@") do not factor (their separator can form across a token boundary): UER is still counted on the device, the
word counts come from `count_errors_host` -- the reference's loop on strings with a pure-Python Levenshtein -- with a one-time warning.
`count_errors_host` is also the statement of the contract for CPU tensors."""
import warnings

import torch

from .task import post_process as _post_process

TABLE_MODES = (None, "none", "letter", "sentencepiece", "wordpiece")
_SEPARATOR = {"letter": "|", "sentencepiece": "▁", "wordpiece": "_"}
KEYS = ("c_errors", "c_total", "w_errors", "wv_errors", "w_total")


def symbol_bytes(dictionary, mode):
    """The per-symbol byte strings g(i) of the docstring, a list of len(dictionary) `bytes`.  Reads dictionary[i] and the special
    indices only."""
    if mode not in TABLE_MODES:
        raise ValueError(f"post_process mode {mode!r} does not factor per symbol")
    bos, eos, unk = dictionary.bos(), dictionary.eos(), dictionary.unk()
    sep = _SEPARATOR.get(mode)
    out = []
    for i in range(len(dictionary)):
        if i == bos or i == eos:
            out.append(b"")
            continue
        s = "<unk>" if i == unk else str(dictionary[i])
        s = s + " " if sep is None else s.replace(" ", "").replace(sep, " ")
        out.append("".join(" " if ch.isspace() else ch for ch in s).encode("utf-8"))
    return out


class ByteTable:
    """symbol_bytes on a device: offsets int32 [V + 1] into data uint8."""

    def __init__(self, strings, device):
        offsets = [0]
        for s in strings:
            offsets.append(offsets[-1] + len(s))
        self.V = len(strings)
        self.max_symbol_bytes = max((len(s) for s in strings), default=0)
        # a word of a sentence starts at a word start of one of its symbols: a sentence of L tokens holds at most L * this many words
        self.max_symbol_words = max((len(s.split()) for s in strings), default=0)
        self.offsets = torch.tensor(offsets, dtype=torch.int32, device=device)
        self.data = torch.tensor(list(b"".join(strings)), dtype=torch.uint8, device=device)


def byte_table(dictionary, mode, device, cache=None):
    """The table of (dictionary, mode) on `device`.  cache: a dict of the caller's (the criterion keeps one) in which the table is kept
    under the mode, the device and the dictionary's symbols themselves, so a dictionary that grows or changes in place gets a new table
    and nothing outlives its owner.  The key is rebuilt from every symbol on each call and a miss drops the other entries: on purpose --
    a few microseconds at the recipes' 81 symbols, one mode per criterion, and no stale table can survive."""
    device = torch.device(device)
    if cache is None:
        return ByteTable(symbol_bytes(dictionary, mode), device)
    key = (mode, device.type, device.index, tuple(str(dictionary[i]) for i in range(len(dictionary))))
    tab = cache.get(key)
    if tab is None:
        cache.clear()
        tab = cache[key] = ByteTable(symbol_bytes(dictionary, mode), device)
    return tab


def strip_pad_eos(target, pad, eos):
    """Target rows with pad and eos removed, order kept: int32 [B, L] (left-packed) and int32 lengths [B].  Device ops, no host read."""
    B, L = target.shape
    keep = (target != pad) & (target != eos)
    pos = torch.where(keep, keep.cumsum(-1) - 1, torch.full_like(target, L, dtype=torch.long))
    rows = torch.zeros(B, L + 1, dtype=torch.int32, device=target.device)
    rows.scatter_(1, pos, target.to(torch.int32))
    return rows[:, :L].contiguous(), keep.sum(-1).to(torch.int32)


def levenshtein(a, b):
    """editdistance.eval for two sequences of comparable items (unit costs).  (Written out again in tests/asr_metrics_reference.py and
    tools/make_golden_wer.py on purpose: the test reference and the golden's stand-in for `editdistance` must not import the code
    they check.)"""
    a, b = list(a), list(b)
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (x != y))
    return row[-1]


def _string(dictionary, tokens):
    """fairseq Dictionary.string(tokens) with its defaults, from dictionary[i] and the special indices only."""
    bos, eos, unk = dictionary.bos(), dictionary.eos(), dictionary.unk()
    return " ".join("<unk>" if t == unk else str(dictionary[t]) for t in tokens if t != bos and t != eos)


def greedy_units_host(lprobs_tv, blank):
    """speech_to_text_loss.py:271-272 on one sentence's [T_b, V] posterior."""
    if lprobs_tv.size(0) == 0:
        return []
    toks = lprobs_tv.argmax(dim=-1).unique_consecutive()
    return toks[toks != blank].tolist()


def count_errors_host(lprobs, input_lengths, target, dictionary, blank, post_process="sentencepiece", pred_units=None):
    """The reference's loop (speech_to_text_loss.py:235-297 without the KenLM decoder) on host copies: lprobs [T, B, V], input_lengths
    [B], target [B, L] with pad / eos anywhere.  -> dict of the five Python ints.  pred_units: per-sentence lists of already decoded
    units (then lprobs and input_lengths are not read)."""
    pad, eos = dictionary.pad(), dictionary.eos()
    out = dict.fromkeys(KEYS, 0)
    target = target.detach().cpu()
    if pred_units is None:
        lp = lprobs.detach().transpose(0, 1).float().contiguous().cpu()
        lens = [min(max(int(n), 0), lp.size(1)) for n in input_lengths.detach().cpu().tolist()]
        pred_units = [greedy_units_host(lp[b, :lens[b]], blank) for b in range(lp.size(0))]
    for pred, t in zip(pred_units, target):
        targ = [int(x) for x in t.tolist() if x != pad and x != eos]
        out["c_errors"] += levenshtein(pred, targ)
        out["c_total"] += len(targ)
        targ_words = _post_process(_string(dictionary, targ), post_process).split()
        pred_words = _post_process(_string(dictionary, pred), post_process).split()
        dist = levenshtein(pred_words, targ_words)
        out["w_errors"] += dist
        out["wv_errors"] += dist
        out["w_total"] += len(targ_words)
    return out


_warned = set()


def _warn_once(key, message):
    if key not in _warned:
        _warned.add(key)
        warnings.warn(message)


def count_errors_rows(lprobs, input_lengths, target, dictionary, blank, post_process="sentencepiece", tables=None):
    """Per sentence: dict of int32 [B] device tensors c_errors, c_total, w_errors, w_total, and the int32 [1] flag that a token id
    outside the dictionary was met (such a token contributes no bytes to the words).  No host read in the table modes."""
    from . import functional as Fn
    if not lprobs.is_cuda:
        raise RuntimeError(f"asr_metrics.count_errors runs on the GPU (csrc/asr_metrics.hip); got lprobs on {lprobs.device} -- "
                           "count_errors_host states the same contract for CPU tensors")
    dev = lprobs.device
    target = target.to(dev)
    pred, pred_len = Fn.ctc_greedy_rows(lprobs, input_lengths, blank)
    tgt, tgt_len = strip_pad_eos(target, dictionary.pad(), dictionary.eos())
    out = {"c_errors": Fn.edit_distance_rows(pred, pred_len, tgt, tgt_len), "c_total": tgt_len}
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    if post_process in TABLE_MODES:
        tab = byte_table(dictionary, post_process, dev, tables)
        pw = Fn.tokens_to_words(pred, pred_len, tab.offsets, tab.data, tab.max_symbol_bytes, err)
        tw = Fn.tokens_to_words(tgt, tgt_len, tab.offsets, tab.data, tab.max_symbol_bytes, err)
        p_ids, t_ids = Fn.word_ids(pw, tw)
        # (the id rows are as wide as the bytes allow; the word counts cannot pass tokens * words per symbol)
        p_ids = p_ids[:, :pred.size(1) * tab.max_symbol_words].contiguous()
        t_ids = t_ids[:, :tgt.size(1) * tab.max_symbol_words].contiguous()
        out["w_errors"] = Fn.edit_distance_rows(p_ids, pw.n, t_ids, tw.n)
        out["w_total"] = tw.n
    else:
        _warn_once(("mode", post_process), f"post_process = {post_process!r} does not factor per symbol: the validation word counts are "
                   "computed on the host (one device-to-host copy of the decoded units per validation step)")
        rows = [row[:k] for row, k in zip(pred.tolist(), pred_len.tolist())]
        host = [count_errors_host(None, None, target[b:b + 1], dictionary, blank, post_process, pred_units=rows[b:b + 1])
                for b in range(len(rows))]
        out["w_errors"] = torch.tensor([h["w_errors"] for h in host], dtype=torch.int32, device=dev)
        out["w_total"] = torch.tensor([h["w_total"] for h in host], dtype=torch.int32, device=dev)
    return out, err


def count_errors(lprobs, input_lengths, target, dictionary, blank, post_process="sentencepiece", tables=None):
    """The five sums for lprobs [T, B, V] fp32 on the GPU, input_lengths [B], target [B, L]: int64 device scalars, and the flag of
    count_errors_rows."""
    rows, err = count_errors_rows(lprobs, input_lengths, target, dictionary, blank, post_process, tables)
    out = {k: v.sum(dtype=torch.int64) for k, v in rows.items()}
    out["wv_errors"] = out["w_errors"]
    return out, err
