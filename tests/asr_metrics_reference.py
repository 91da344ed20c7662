"""Pure-Python statement of the four contracts of csrc/asr_metrics.hip and of the five sums of the ASR criterion's validation block
(speech_to_text_loss.py:232-297).  Lists and ints only; tests/test_asr_metrics_cpu.py checks it against the string form of the
reference and against tests/golden/s2t_wer.pt, tests/test_asr_metrics_gpu.py checks the kernels against it.

`fault=` plants one named mistake (tests/test_asr_metrics_cpu.py shows that the suite catches each):
  "blank_first"   blanks dropped before the collapse        "last_tie"   ties resolved to the last index
  "keep_eos"      eos kept in the word string               "hi_off"     the diagonal's upper bound one short
  "sub_equal"     a substitution cost on equal tokens

The table rule and the Levenshtein distance are written out here again, next to speecht5_amd/asr_metrics.py's, on purpose: the reference
imports nothing of the code it checks; both are pinned to `post_process(_Dictionary.string(...))` and to the verbatim criterion's golden."""
import math

SEPARATOR = {"letter": "|", "sentencepiece": "▁", "wordpiece": "_"}
TABLE_MODES = (None, "none", "letter", "sentencepiece", "wordpiece")


# ---- 1. greedy decoding ----
def argmax(row, fault=None):
    """torch's CPU argmax of a list of floats: the lowest index among equal maxima; a NaN beats every number, the first NaN wins."""
    best = 0
    for i in range(1, len(row)):
        x, y = row[i], row[best]
        if math.isnan(y):
            break
        if math.isnan(x) or x > y or (fault == "last_tie" and x == y):
            best = i
    return best


def collapse(best, blank, fault=None):
    """unique_consecutive, then blanks dropped: frame t is kept iff best[t] != blank and (t == 0 or best[t] != best[t - 1])."""
    if fault == "blank_first":
        best = [c for c in best if c != blank]
    return [c for t, c in enumerate(best) if c != blank and (t == 0 or c != best[t - 1])]


def greedy(frames, length, blank, fault=None):
    """frames: T rows of V floats (one sentence); frames at or behind clamp(length, 0, T) are not read."""
    n = min(max(int(length), 0), len(frames))
    return collapse([argmax(list(r), fault) for r in frames[:n]], blank, fault)


# ---- 2. the byte table, the word split, word ids ----
def symbol_bytes(symbols, bos, eos, unk, mode, fault=None):
    """Per-symbol byte strings (speecht5_amd/asr_metrics.py states the rule): symbols is the whole dictionary as a list of str."""
    assert mode in TABLE_MODES
    sep = SEPARATOR.get(mode)
    out = []
    for i, s in enumerate(symbols):
        if i == bos or (i == eos and fault != "keep_eos"):
            out.append(b"")
            continue
        s = "<unk>" if i == unk else s
        s = s + " " if sep is None else s.replace(" ", "").replace(sep, " ")
        out.append("".join(" " if ch.isspace() else ch for ch in s).encode("utf-8"))
    return out


def words(tokens, table):
    """-> (list of the sentence's words as bytes, flag: a token outside [0, V) was met; it contributes no bytes)."""
    bad = any(not 0 <= t < len(table) for t in tokens)
    sent = b"".join(table[t] for t in tokens if 0 <= t < len(table))
    return [w for w in sent.split(b" ") if w], bad


def word_ids(pred_words, targ_words):
    """Ids with id(pred) == id(targ) iff equal bytes and id(targ) == id(targ) iff equal bytes: a target word gets the index of its first
    occurrence, a predicted word that of the first equal target word, else len(targ_words) + its own index."""
    t_ids = [targ_words.index(w) for w in targ_words]
    p_ids = [targ_words.index(w) if w in targ_words else len(targ_words) + i for i, w in enumerate(pred_words)]
    return p_ids, t_ids


# ---- 3. Levenshtein distance ----
def levenshtein(a, b, fault=None):
    """Row form, unit costs (editdistance.eval)."""
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            sub = prev + (1 if (x != y or fault == "sub_equal") else 0)
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, sub)
    return row[-1]


def levenshtein_diagonals(a, b, fault=None):
    """The kernel's form: anti-diagonals k = i + j with i along the SHORTER sequence, three rotating diagonals in ONE list addressed
    as (k % 3) * stride + i, stride = min(n, m) + 1.  Unwritten slots hold None, so a read of a cell that is not there fails."""
    sh, lg = (b, a) if len(a) > len(b) else (a, b)
    s, l = len(sh), len(lg)
    stride = s + 1
    buf = [None] * (3 * stride)

    def off(k, i):
        assert 0 <= i < stride
        return (k % 3) * stride + i
    for k in range(s + l + 1):
        lo, hi = max(0, k - l), min(k, s)
        if fault == "hi_off":
            hi = min(k, s - 1) if s else hi
        for i in range(lo, hi + 1):
            j = k - i
            if i == 0:
                d = j
            elif j == 0:
                d = i
            else:
                up, left, diag = buf[off(k - 1, i - 1)], buf[off(k - 1, i)], buf[off(k - 2, i - 1)]
                d = min(min(up, left) + 1, diag + (1 if (sh[i - 1] != lg[j - 1] or fault == "sub_equal") else 0))
            buf[off(k, i)] = d
        for i in list(range(0, lo)) + list(range(hi + 1, stride)):
            buf[off(k, i)] = None      # (what the kernel leaves there is stale: never read)
    return buf[off(s + l, s)]


# ---- 4. the five sums ----
def sentence_counts(pred_units, target, pad, eos, table, fault=None):
    """-> (c_errors, c_total, w_errors, w_total) of one sentence; target: token ids with pad / eos anywhere."""
    targ = [int(t) for t in target if t != pad and t != eos]
    pw, _ = words(pred_units, table)
    tw, _ = words(targ if fault != "keep_eos" else [int(t) for t in target if t != pad], table)
    p_ids, t_ids = word_ids(pw, tw)
    return levenshtein_diagonals(pred_units, targ, fault), len(targ), levenshtein_diagonals(p_ids, t_ids, fault), len(tw)


def five_sums(lprobs, input_lengths, targets, blank, pad, eos, table, fault=None):
    """lprobs: nested lists [T][B][V]; targets: B lists of ids.  -> (dict of the five sums, per-sentence rows)."""
    B = len(targets)
    rows = []
    for b in range(B):
        pred = greedy([frame[b] for frame in lprobs], input_lengths[b], blank, fault)
        rows.append(sentence_counts(pred, targets[b], pad, eos, table, fault))
    tot = [sum(r[j] for r in rows) for j in range(4)]
    return dict(c_errors=tot[0], c_total=tot[1], w_errors=tot[2], wv_errors=tot[2], w_total=tot[3]), [list(r) for r in rows]
