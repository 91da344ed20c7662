"""Validation UER / WER on the GPU (csrc/asr_metrics.hip, speecht5_amd/asr_metrics.py, SpeechtoTextLoss in eval mode) against the
pure-Python reference (tests/asr_metrics_reference.py) and the counts of the VERBATIM reference criterion (tests/golden/s2t_wer.pt).
Every expected value is an integer: all comparisons are exact.  The smallest kernel cases come first."""
import json
import os
import random
import subprocess
import sys

import pytest
import torch

from speecht5_amd.task import _Dictionary
from tests import asr_metrics_reference as R
from tests.util import build_tiny, load_golden, to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = ["<mask>", "<ctc_blank>"]
MODES = [None, "none", "letter", "sentencepiece", "wordpiece"]
SYMBOLS = list("abc") + ["|", "▁", "_", "ab", "▁the", "he|", "_x_", "d e", "t\tu", "v　w", "", "é", "▁é|", " "]


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rows(seqs, dev, width=None):
    L = max([len(s) for s in seqs] + [1]) if width is None else width
    t = torch.full((len(seqs), L), -7, dtype=torch.int32)
    for i, s in enumerate(seqs):
        t[i, :len(s)] = torch.tensor(s, dtype=torch.int32)
    return t.to(dev), torch.tensor([len(s) for s in seqs], dtype=torch.int32, device=dev)


def _distances(pairs, dev, la=None, lb=None):
    from speecht5_amd import functional as Fn
    a, an = _rows([p[0] for p in pairs], dev, la)
    b, bn = _rows([p[1] for p in pairs], dev, lb)
    return Fn.edit_distance_rows(a, an, b, bn).tolist()


# ---- edit distance ----
def test_edit_distance_smallest(cuda):
    pairs = [([], []), ([1], []), ([], [1]), ([1], [1]), ([1], [2]), ([1, 2], [2]), ([1, 2], [1, 2]), ([1, 2], [2, 1]), ([1, 2], [3, 4])]
    assert _distances(pairs, cuda) == [0, 1, 1, 0, 1, 1, 0, 2, 2]
    assert _distances(pairs, cuda) == [R.levenshtein(a, b) for a, b in pairs]


def test_edit_distance_random_sweep(cuda):
    rng = random.Random(7)
    pairs = []
    for _ in range(200):
        a = [rng.randrange(4) for _ in range(rng.randint(0, 40))]
        b = [rng.randrange(4) for _ in range(rng.randint(0, 40))] if rng.random() < 0.6 else a[rng.randint(0, 3):] + [rng.randrange(4)]
        pairs.append((a, b))
    assert _distances(pairs, cuda) == [R.levenshtein_diagonals(a, b) for a, b in pairs]


# ---- greedy decoding ----
def _posterior(paths, lengths, V, seed):
    """[T, B, V] whose argmax follows paths[b][t]."""
    g = torch.Generator().manual_seed(seed)
    B, T = len(paths), len(paths[0])
    lp = torch.randn(T, B, V, generator=g)
    idx = torch.tensor(paths, dtype=torch.long).t().unsqueeze(-1)
    lp.scatter_add_(2, idx, torch.full(idx.shape, 20.0))
    return lp


def _greedy_expected(lp, lengths, blank):
    T, B, _ = lp.shape
    best = lp.argmax(-1).t().tolist()          # torch's CPU rule (tests/test_asr_metrics_cpu.py pins the reference's to it)
    pred, n = torch.full((B, T), -1, dtype=torch.int32), []
    for b in range(B):
        u = R.collapse(best[b][:min(max(int(lengths[b]), 0), T)], blank)
        pred[b, :len(u)] = torch.tensor(u, dtype=torch.int32)
        n.append(len(u))
    return pred, n


@pytest.mark.parametrize("V", [3, 81, 300])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 257, 513])
def test_greedy_rows(cuda, T, V):
    from speecht5_amd import functional as Fn
    rng = random.Random(T * 1000 + V)
    B, blank = 7, V - 1
    lengths = [T, 0, T // 2, max(T - 1, 0), T + 5, -3, 1]         # ragged; 0 and T; above T and negative are clamped
    paths = [[rng.randrange(V) if rng.random() < 0.7 else blank for _ in range(T)] for _ in range(B)]
    for t0 in range(255, T - 1, 256):        # every chunk boundary of the compaction (chunks of 256 frames)
        paths[0][t0] = paths[0][t0 + 1] = 0                       # a repeated unit straddles it: one unit
        paths[3][t0], paths[3][t0 + 1] = blank, 1                 # blank | unit
        paths[4][t0], paths[4][t0 + 1] = 1, 0                     # two different units
    paths[6] = [blank] * T                                        # all blank
    lp = _posterior(paths, lengths, V, seed=T + V)
    nan, inf = float("nan"), float("inf")
    if T >= 2:
        lp[0, 2, :] = lp[0, 2, 0]            # a frame of ties: class 0
        lp[1, 2, :] = -inf                   # a frame of -inf: class 0
        lp[1, 3, V // 2] = nan               # a NaN wins
        lp[0, 4, 1:] = nan                   # the first NaN wins
        lp[1, 0, V - 1] = lp[1, 0, 0] = 50.0 # a tie between the first and the last class
    want, want_n = _greedy_expected(lp, lengths, blank)
    pred, n = Fn.ctc_greedy_rows(lp.to(cuda), torch.tensor(lengths, device=cuda), blank)
    assert pred.dtype == torch.int32 and n.dtype == torch.int32 and pred.shape == (B, T)
    assert n.tolist() == want_n
    assert torch.equal(pred.cpu(), want)


def test_greedy_a_blank_between_equal_units_keeps_both(cuda):
    from speecht5_amd import functional as Fn
    paths = [[0, 2, 0, 0, 2, 2, 1, 1, 0]]
    pred, n = Fn.ctc_greedy_rows(_posterior(paths, [9], 3, 1).to(cuda), torch.tensor([9], device=cuda), 2)
    assert pred[0, :int(n)].tolist() == [0, 0, 1, 0]


def test_greedy_one_frame_nan_tie_and_minus_inf(cuda):
    """The argmax rule at the smallest shape: T = 1, one row per special frame, each inside its length."""
    from speecht5_amd import functional as Fn
    nan, inf = float("nan"), float("inf")
    frames = [[1.0, nan, 2.0, nan, 0.0], [3.0, 1.0, 3.0, 3.0, 0.0], [-inf] * 5, [0.0, 1.0, 2.0, 3.0, nan], [-1.0, -inf, -1.0, -2.0, -3.0],
              [nan] * 5]
    lp = torch.tensor(frames).unsqueeze(0)                  # [1, 6, 5]
    want = [R.argmax(f) for f in frames]
    assert want == lp[0].argmax(-1).tolist() == [1, 0, 0, 4, 0, 0]
    pred, n = Fn.ctc_greedy_rows(lp.to(cuda), torch.ones(6, dtype=torch.long, device=cuda), 9)
    assert n.tolist() == [1] * 6 and pred[:, 0].tolist() == want


# ---- words ----
def _device_words(tokens, table, dev):
    from speecht5_amd import asr_metrics as A
    from speecht5_amd import functional as Fn
    tab = A.ByteTable(table, dev)
    rows, lens = _rows(tokens, dev)
    return Fn.tokens_to_words(rows, lens, tab.offsets, tab.data, tab.max_symbol_bytes)


def _words_of(w, b):
    raw = bytes(w.bytes[b].tolist())
    return [raw[s:s + n] for s, n in zip(w.start[b, :int(w.n[b])].tolist(), w.len[b, :int(w.n[b])].tolist())]


@pytest.mark.parametrize("mode", MODES)
def test_words_in_every_table_mode(cuda, mode):
    from speecht5_amd import functional as Fn
    d = _Dictionary(SYMBOLS, EXTRA)
    table = R.symbol_bytes(list(d), d.bos(), d.eos(), d.unk(), mode)
    rng = random.Random(len(str(mode)))
    tokens = [[rng.randrange(len(d)) for _ in range(rng.randint(0, 40))] for _ in range(12)]
    tokens += [[], [d.bos(), d.eos(), d.pad(), d.unk()], [rng.randrange(len(d)) for _ in range(300)]]     # 300 tokens: several chunks
    w = _device_words(tokens, table, cuda)
    assert int(w.err) == 0
    for b, toks in enumerate(tokens):
        assert _words_of(w, b) == R.words(toks, table)[0], (mode, b)
    # an id outside the dictionary: no bytes, the flag is set, the other rows are right
    bad = [list(t) for t in tokens]
    bad[3] = bad[3][:2] + [len(d)] + bad[3][2:] + [-1, 2 ** 31 - 1]
    w = _device_words(bad, table, cuda)
    assert int(w.err) == 1
    for b, toks in enumerate(tokens):
        assert _words_of(w, b) == R.words(toks, table)[0], (mode, b)
    # ids: predicted against target words of the same sentences (the rows reversed serve as targets)
    targets = [list(reversed(t)) for t in tokens]
    tw = _device_words(targets, table, cuda)
    w = _device_words(tokens, table, cuda)
    p_ids, t_ids = Fn.word_ids(w, tw)
    for b in range(len(tokens)):
        pw, tws = R.words(tokens[b], table)[0], R.words(targets[b], table)[0]
        pi, ti = p_ids[b, :len(pw)].tolist(), t_ids[b, :len(tws)].tolist()
        assert all((x == y) == (ix == iy) for x, ix in zip(pw, pi) for y, iy in zip(tws, ti))
        assert all((x == y) == (ix == iy) for x, ix in zip(tws, ti) for y, iy in zip(tws, ti))
        assert (pi, ti) == R.word_ids(pw, tws)


def test_two_tokenisations_of_a_word_get_one_id(cuda):
    from speecht5_amd import functional as Fn
    d = _Dictionary(["a", "b", "ab", "|", "é", "éa"], EXTRA)
    ix = d.index
    table = R.symbol_bytes(list(d), d.bos(), d.eos(), d.unk(), "letter")
    pred = [[ix("a"), ix("b"), ix("|"), ix("é"), ix("a"), ix("|"), ix("b")], [], [ix("|"), ix("|")]]
    targ = [[ix("ab"), ix("|"), ix("éa"), ix("|"), ix("a")], [ix("ab")], []]
    pw, tw = _device_words(pred, table, cuda), _device_words(targ, table, cuda)
    assert _words_of(pw, 0) == [b"ab", "éa".encode(), b"b"] and _words_of(tw, 0) == [b"ab", "éa".encode(), b"a"]
    assert pw.n.tolist() == [3, 0, 0] and tw.n.tolist() == [3, 1, 0]
    p_ids, t_ids = Fn.word_ids(pw, tw)
    assert p_ids[0, :2].tolist() == t_ids[0, :2].tolist() and int(p_ids[0, 2]) not in t_ids[0, :3].tolist()
    assert Fn.edit_distance_rows(p_ids, pw.n, t_ids, tw.n).tolist() == [1, 1, 0]


# ---- edit distance, the larger cases ----
def test_edit_distance_lengths_around_the_block_and_wave_sizes(cuda):
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257]
    rng = random.Random(8)
    base = [rng.randrange(5) for _ in range(257)]
    other = [rng.randrange(5) for _ in range(257)]
    pairs = [(base[:n], other[:m]) for n in sizes for m in sizes]
    assert _distances(pairs, cuda) == [R.levenshtein(a, b) for a, b in pairs]
    # equal, disjoint and shifted sequences: known distances
    eq = [(base[:n], base[:n]) for n in sizes]
    dj = [(list(range(n)), list(range(1000, 1000 + m))) for n in sizes for m in (0, 64, 257)]
    sh = [(list(range(n)), list(range(1, n + 1))) for n in sizes]
    assert _distances(eq, cuda) == [0] * len(sizes)
    assert _distances(dj, cuda) == [max(len(a), len(b)) for a, b in dj]
    assert _distances(sh, cuda) == [min(n, 2) for n in sizes]


def test_edit_distance_long_sides_lengths_clamped_and_the_refusal(cuda):
    from speecht5_amd import functional as Fn
    rng = random.Random(9)
    long_a, short = [rng.randrange(3) for _ in range(4095)], [rng.randrange(3) for _ in range(7)]
    long_b = [rng.randrange(3) for _ in range(1500)]
    assert _distances([(long_a, short)], cuda) == [R.levenshtein(long_a, short)]
    assert _distances([(short, long_b)], cuda) == [R.levenshtein(short, long_b)]
    # the largest LDS footprint (three diagonals of 4096 ints): equal, shifted by one, disjoint
    n = 4095
    assert _distances([(list(range(n)), list(range(n))), (list(range(n)), list(range(1, n + 1))),
                       (list(range(n)), list(range(5000, 5000 + n)))], cuda) == [0, 2, n]
    # lengths outside their rows are clamped: nothing behind a row is read
    a, _ = _rows([[1, 2, 3], [1, 2, 3]], cuda)
    b, _ = _rows([[1, 2, 4], [9, 9, 9]], cuda)
    wild = torch.tensor([100, -5], dtype=torch.int32, device=cuda)
    assert Fn.edit_distance_rows(a, wild, b, torch.tensor([3, 2], dtype=torch.int32, device=cuda)).tolist() == [1, 2]
    # min(La, Lb) = 4096: refused in Python, nothing launched
    z = torch.zeros(1, 4096, dtype=torch.int32, device=cuda)
    one = torch.ones(1, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError):
        Fn.edit_distance_rows(z, one, z, one)
    assert Fn.edit_distance_rows(z, one, z[:, :4095].contiguous(), one).tolist() == [0]


# ---- the counts ----
def _golden_cases():
    return torch.load(os.path.join(ROOT, "tests", "golden", "s2t_wer.pt"), weights_only=False)["cases"]


def _reference_rows(lp, lengths, target, d, blank, mode):
    table = R.symbol_bytes(list(d), d.bos(), d.eos(), d.unk(), mode)
    return R.five_sums(lp.tolist(), [int(x) for x in lengths], target.tolist(), blank, d.pad(), d.eos(), table)


def _device_rows(lp, lengths, target, d, blank, mode, dev):
    from speecht5_amd import asr_metrics as A
    rows, err = A.count_errors_rows(lp.to(dev), torch.as_tensor(lengths).to(dev), target.to(dev), d, blank, mode)
    return [list(r) for r in zip(*(rows[k].tolist() for k in ("c_errors", "c_total", "w_errors", "w_total")))], int(err)


def test_kernels_reproduce_the_verbatim_criterion(cuda):
    from speecht5_amd import asr_metrics as A
    for case in _golden_cases():
        d = _Dictionary(case["symbols"], EXTRA)
        rows, err = _device_rows(case["lprobs"], case["input_lengths"], case["target_label"], d, case["blank"], case["mode"], cuda)
        assert rows == case["rows"] and err == 0, (case["mode"], rows, case["rows"])
        sums, _ = A.count_errors(case["lprobs"].to(cuda), case["input_lengths"].to(cuda), case["target_label"].to(cuda), d, case["blank"],
                                 case["mode"])
        assert all(v.dtype == torch.int64 and v.dim() == 0 and v.is_cuda for v in sums.values())
        assert {k: int(v) for k, v in sums.items()} == case["counts"]


def test_a_rows_counts_do_not_depend_on_the_other_rows(cuda):
    d = _Dictionary(list("abcdefg") + ["|"], EXTRA)
    blank, V, T, B, L = d.index("<ctc_blank>"), len(d), 300, 6, 40
    g = torch.Generator().manual_seed(13)
    lp = torch.log_softmax(torch.randn(T, B, V, generator=g) * 2, -1)
    lp[:, :, blank] += 1.5
    lengths = torch.tensor([300, 17, 0, 257, 256, 299])
    target = torch.randint(1, V - 2, (B, L), generator=g)
    want, _ = _device_rows(lp, lengths, target, d, blank, "letter", cuda)
    assert want == _reference_rows(lp, lengths, target, d, blank, "letter")[1]
    perm = [4, 0, 5, 2, 1, 3]
    got, _ = _device_rows(lp[:, perm].contiguous(), lengths[perm], target[perm], d, blank, "letter", cuda)
    assert got == [want[p] for p in perm]
    lp2, len2, tg2 = lp.clone(), lengths.clone(), target.clone()
    lp2[:, 1:] = torch.log_softmax(torch.randn(T, B - 1, V, generator=g), -1)
    len2[1:], tg2[1:] = 300, 5
    assert _device_rows(lp2, len2, tg2, d, blank, "letter", cuda)[0][0] == want[0]
    assert _device_rows(lp[:, 3:4].contiguous(), lengths[3:4], target[3:4], d, blank, "letter", cuda)[0] == [want[3]]


def test_modes_that_do_not_factor_count_words_on_the_host(cuda):
    from speecht5_amd import asr_metrics as A
    d = _Dictionary(["a@@", "b", "c@@", "d"], EXTRA)
    blank = d.index("<ctc_blank>")
    g = torch.Generator().manual_seed(3)
    lp = torch.log_softmax(torch.randn(20, 3, len(d), generator=g) * 3, -1)
    lengths, target = torch.tensor([20, 11, 0]), torch.randint(2, 8, (3, 6), generator=g)
    with pytest.warns(UserWarning):
        A._warned.clear()
        got, _ = A.count_errors(lp.to(cuda), lengths.to(cuda), target.to(cuda), d, blank, "subword_nmt")
    assert {k: int(v) for k, v in got.items()} == A.count_errors_host(lp, lengths, target, d, blank, "subword_nmt")


# ---- model level ----
_CHILD = r'''
import json, sys
import speecht5_amd
from speecht5_amd import fairseq_compat as fc
from speecht5_amd.criterions import SpeechT5Criterion
from fairseq.logging import metrics
assert fc.HAVE_FAIRSEQ
SpeechT5Criterion.reduce_metrics(json.load(open(sys.argv[1])))
print("CALLS " + json.dumps(metrics.CALLS))
'''


def test_valid_step_reports_the_counts(cuda, tmp_path):
    from types import SimpleNamespace
    from speecht5_amd import fairseq_compat as fc
    from speecht5_amd import hip
    from speecht5_amd.criterions import SpeechT5Criterion, SpeechtoTextLoss
    from speecht5_amd.task import SpeechT5Task
    _, fx = load_golden("tiny_s2t.pt")
    model, args = build_tiny(cuda, torch.float32)
    # a _Dictionary of the tiny model's layout: 4 specials + 30 symbols + <mask> + <ctc_blank>
    d = _Dictionary(list("abcdefghijklmnopqrstuvwxyz") + ["|", "'", "é", "-"])
    task = SpeechT5Task(args, {"text": d})
    sample = to_dev(fx["sample"], cuda)
    sample["task_name"] = "s2t"
    bar = d.index("|")
    label = sample["target"].clone()
    label[:, 2::4] = bar                                    # several words per target
    sample["target_label"] = torch.where(sample["target"] == d.pad(), sample["target"], label)
    cfg = SimpleNamespace(zero_infinity=True, post_process="letter")
    crit = SpeechT5Criterion(task, sentence_avg=False, ce_weight=0.5, ctc_weight=0.5, cfg=cfg)
    seen = {}
    inner = SpeechtoTextLoss._ctc_inputs

    def spy(self, m, net_output):
        out = inner(self, m, net_output)
        seen["lprobs"], seen["lengths"] = out[0].detach().cpu(), out[1].detach().cpu()
        return out
    SpeechtoTextLoss._ctc_inputs = spy
    calls, lib = [], hip.lib

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib(), name)
            if name.startswith("st5_"):
                calls.append(name)
            return fn
    hip.lib = lambda: Counting()
    try:
        _, _, log = task.valid_step(sample, model, crit)
        eval_calls = list(calls)
        del calls[:]
        model.train()
        _, _, train_log = crit(model, sample)
        train_calls = list(calls)
        crit.text_criterion.sync_logging = False
        _, _, dev_log = task.valid_step(sample, model, crit)
    finally:
        SpeechtoTextLoss._ctc_inputs = inner
        hip.lib = lib
    keys = ("c_errors", "c_total", "w_errors", "wv_errors", "w_total")
    assert all(isinstance(log[k], int) for k in keys), {k: log.get(k) for k in keys}
    # the step's own posterior on the host: ties resolve identically
    want, _ = _reference_rows(seen["lprobs"], seen["lengths"], sample["target_label"].cpu(), d, d.index("<ctc_blank>"), "letter")
    assert seen["lprobs"].size(2) == len(d)
    assert {k: log[k] for k in keys} == want
    assert log["c_total"] > 0 and log["w_total"] > log["nsentences"]
    # training mode: none of the keys, none of the kernels; eval mode adds exactly the four entry points
    assert not any(k in train_log for k in keys)
    ours = {"st5_ctc_greedy_rows", "st5_tokens_to_words", "st5_word_ids", "st5_edit_distance_rows"}
    assert not ours & set(train_calls)
    assert [c for c in eval_calls if c in ours] == ["st5_ctc_greedy_rows", "st5_edit_distance_rows", "st5_tokens_to_words",
                                                    "st5_tokens_to_words", "st5_word_ids", "st5_edit_distance_rows"]
    # sync_logging=False: int64 device scalars with the same values
    assert all(torch.is_tensor(dev_log[k]) and dev_log[k].is_cuda and dev_log[k].dtype == torch.int64 and dev_log[k].dim() == 0 for k in keys)
    assert {k: int(dev_log[k]) for k in keys} == want
    # through reduce_metrics: the in-tree metrics give the rates, a fairseq that enforces its interfaces takes the same calls
    fc.metrics.reset()
    SpeechT5Criterion.reduce_metrics([{"s2t": log}])
    derived = {k: fn(fc.metrics.meters) for k, fn in fc.metrics.derived.items()}
    assert derived["uer"] == fc.safe_round(log["c_errors"] * 100.0 / log["c_total"], 3)
    assert derived["wer"] == derived["raw_wer"] == fc.safe_round(log["w_errors"] * 100.0 / log["w_total"], 3)
    path = tmp_path / "log.json"
    path.write_text(json.dumps([{"s2t": {k: v for k, v in log.items() if isinstance(v, (int, float))}}]))
    fake = os.path.join(ROOT, "tests", "fake_fairseq")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([fake, ROOT, os.environ.get("PYTHONPATH", "")]), HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _CHILD, str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CALLS " in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    recorded = json.loads(out.stdout[out.stdout.index("CALLS ") + 6:].splitlines()[0])
    scalars = {c[1]: c[2] for c in recorded if c[0] == "scalar"}
    assert {k: int(scalars["_" + k]) for k in keys} == want
    assert {"uer", "wer", "raw_wer"} <= {c[1] for c in recorded if c[0] == "derived"}
