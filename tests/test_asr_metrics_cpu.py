"""Validation UER / WER without a GPU:
1. the Python reference (tests/asr_metrics_reference.py) against the reference's string form
   `post_process(_Dictionary.string(tokens), mode).split()` in the five table modes, and against tests/golden/s2t_wer.pt (counts the
   VERBATIM reference criterion logged, tools/make_golden_wer.py);
2. the anti-diagonal three-buffer Levenshtein form against the row form;
3. csrc/asr_metrics_index.h compiled with the host compiler: every offset its helpers produce lies inside its buffer, and the cell order
   visits each (i, j) once with its three predecessors in place;
4. speecht5_amd.asr_metrics (symbol_bytes, count_errors_host, strip_pad_eos) against the reference;
5. five planted faults that the checks above must catch;
6. the compiled kernels of asr_metrics.hip reach LDS with ds_* instructions only and use no scratch."""
import os
import random
import shutil
import subprocess

import pytest
import torch

from speecht5_amd import asr_metrics as A
from speecht5_amd.task import _Dictionary, post_process
from tests import asr_metrics_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = ["<mask>", "<ctc_blank>"]
MODES = [None, "none", "letter", "sentencepiece", "wordpiece"]
# single letters, the three separators, multi-character symbols, symbols holding a space / a tab / U+3000, the empty string, a
# multi-byte letter, symbols that glue separators to letters
SYMBOLS = list("abc") + ["|", "▁", "_", "ab", "▁the", "he|", "_x_", "d e", "t\tu", "v　w", "", "é", "▁é|", " "]


def golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "s2t_wer.pt"), weights_only=False)


def table_of(d, mode, fault=None):
    return R.symbol_bytes(list(d), d.bos(), d.eos(), d.unk(), mode, fault)


def golden_counts(case, fault=None):
    d = _Dictionary(case["symbols"], EXTRA)
    table = table_of(d, case["mode"], fault)
    targets = [[int(x) for x in row] for row in case["target_label"].tolist()]
    return R.five_sums(case["lprobs"].tolist(), case["input_lengths"].tolist(), targets, case["blank"], d.pad(), d.eos(), table, fault)


# ---- 1 ----
def test_argmax_rule_is_torchs():
    nan = float("nan")
    rows = [[nan, 1, 2], [1, 1, 0], [0, nan, nan], [-float("inf")] * 4, [0.0, -0.0, 0.0], [3.0], [1, 2, 2, nan, 5, nan]]
    rng = random.Random(0)
    for _ in range(300):
        rows.append([rng.choice([0.0, 1.0, -1.0, 2.0, nan, float("inf"), -float("inf")]) for _ in range(rng.randint(1, 9))])
    for r in rows:
        assert R.argmax(r) == int(torch.tensor(r).argmax()), r
    assert [R.argmax(r) for r in rows[:3]] == [0, 0, 1]


def test_collapse_is_unique_consecutive_then_blank_removal():
    rng = random.Random(1)
    assert R.collapse([5, 9, 5], 9) == [5, 5]
    for _ in range(300):
        best = [rng.randint(0, 3) for _ in range(rng.randint(0, 12))]
        t = torch.tensor(best, dtype=torch.long).unique_consecutive()
        assert R.collapse(best, 2) == t[t != 2].tolist()


@pytest.mark.parametrize("mode", MODES)
def test_table_words_equal_the_string_form(mode):
    d = _Dictionary(SYMBOLS, EXTRA)
    table = table_of(d, mode)
    assert table == A.symbol_bytes(d, mode)
    rng = random.Random(hash(str(mode)) & 0xFFFF)
    for _ in range(3000):
        toks = [rng.randrange(len(d)) for _ in range(rng.randint(0, 14))]
        got, bad = R.words(toks, table)
        want = post_process(d.string(toks), mode).split()
        assert not bad and got == [w.encode("utf-8") for w in want], (mode, toks, got, want)
    assert R.words([4, -1, len(d), 5], table) == (R.words([4, 5], table)[0], True)


def test_word_ids_compare_bytes():
    rng = random.Random(2)
    vocab = [b"a", b"b", b"ab", b"ba", b"abc", b"\xc3\xa9"]
    for _ in range(500):
        p = [rng.choice(vocab) for _ in range(rng.randint(0, 7))]
        t = [rng.choice(vocab) for _ in range(rng.randint(0, 7))]
        pi, ti = R.word_ids(p, t)
        for x, ix in zip(p, pi):
            for y, iy in zip(t, ti):
                assert (x == y) == (ix == iy)
        for x, ix in zip(t, ti):
            for y, iy in zip(t, ti):
                assert (x == y) == (ix == iy)
        assert R.levenshtein(pi, ti) == R.levenshtein(p, t)


def test_python_reference_reproduces_the_verbatim_criterion():
    for case in golden()["cases"]:
        counts, rows = golden_counts(case)
        assert counts == case["counts"], (case["mode"], counts, case["counts"])
        assert rows == case["rows"], (case["mode"], rows, case["rows"])


# ---- 2 ----
def _pairs(rng, n_pairs, max_len, alphabet):
    for _ in range(n_pairs):
        a = [rng.randrange(alphabet) for _ in range(rng.randint(0, max_len))]
        kind = rng.random()
        if kind < 0.3:
            b = list(a)
            for _ in range(rng.randint(0, 4)):      # a few edits of a
                if b and rng.random() < 0.5:
                    del b[rng.randrange(len(b))]
                else:
                    b.insert(rng.randint(0, len(b)), rng.randrange(alphabet))
        else:
            b = [rng.randrange(alphabet) for _ in range(rng.randint(0, max_len))]
        yield a, b


def test_diagonal_form_equals_row_form():
    rng = random.Random(3)
    for a, b in _pairs(rng, 1500, 14, 3):
        assert R.levenshtein_diagonals(a, b) == R.levenshtein(a, b), (a, b)
    for n in range(0, 9):
        for m in range(0, 9):
            a, b = list(range(n)), list(range(100, 100 + m))
            assert R.levenshtein_diagonals(a, b) == max(n, m)
            assert R.levenshtein_diagonals(a, a[:m]) == max(n - m, 0)
    assert R.levenshtein_diagonals([1, 2, 3, 4], [2, 3, 4, 5]) == 2
    assert R.levenshtein("kitten", "sitting") == 3 and R.levenshtein_diagonals(list("kitten"), list("sitting")) == 3


# ---- 3 ----
SWEEP = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cmath>
#include "asr_metrics_index.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d) n=%d m=%d k=%d i=%d\n", #c, __LINE__, n, m, k, i); return 1; } } while (0)
int main() {
  int n = 0, m = 0, k = 0, i = 0;
  long long cells = 0;
  for (n = 0; n <= 70; ++n) for (m = 0; m <= 70; ++m) for (int extra = 0; extra <= 3; extra += 3) {
    const int s = n < m ? n : m, l = n < m ? m : n;
    const int stride = am_ed_stride(s + extra), size = 3 * stride;
    CHECK(am_ed_lds_bytes(s + extra) == (long long)size * 4);
    std::vector<int> slot(size, -1);              // the cell (i * (l + 1) + j) a slot holds
    std::vector<int> seen((s + 1) * (l + 1), 0);
    for (k = 0; k <= s + l; ++k) {
      const int lo = am_ed_lo(k, l), hi = am_ed_hi(k, s);
      CHECK(lo >= 0 && hi <= s && lo <= hi);
      for (i = lo; i <= hi; ++i) {                // every thread's reads come before the diagonal's barrier
        const int j = k - i;
        CHECK(j >= 0 && j <= l);
        if (i > 0 && j > 0) {
          const int up = am_ed_off(k - 1, i - 1, stride), left = am_ed_off(k - 1, i, stride), diag = am_ed_off(k - 2, i - 1, stride);
          CHECK(up >= 0 && up < size && left >= 0 && left < size && diag >= 0 && diag < size);
          CHECK(slot[up] == (i - 1) * (l + 1) + j);
          CHECK(slot[left] == i * (l + 1) + j - 1);
          CHECK(slot[diag] == (i - 1) * (l + 1) + j - 1);
          CHECK(i - 1 < s && j - 1 < l);          // the token reads sh[i - 1], lg[j - 1]
        }
        const int w = am_ed_off(k, i, stride);
        CHECK(w >= 0 && w < size);
        CHECK(w / stride != ((k + 2) % 3) && w / stride != ((k + 1) % 3));   // not a buffer this diagonal reads
      }
      for (i = lo; i <= hi; ++i) {
        slot[am_ed_off(k, i, stride)] = i * (l + 1) + (k - i);
        ++seen[i * (l + 1) + (k - i)];
        ++cells;
      }
    }
    i = s; k = s + l;
    CHECK(slot[am_ed_off(s + l, s, stride)] == s * (l + 1) + l);
    for (int c = 0; c < (s + 1) * (l + 1); ++c) CHECK(seen[c] == 1);
  }
  // the refusal bound fits the LDS of a workgroup
  CHECK(am_ed_lds_bytes(AM_ED_MAX_SHORT) == 3LL * 4096 * 4 && am_ed_lds_bytes(AM_ED_MAX_SHORT) <= 64 * 1024);
  // caps: L tokens of max_symbol_bytes bytes fill [0, cap) exactly; "x x x ..." holds the most words
  for (int L = 0; L <= 40; ++L) for (int msb = 0; msb <= 9; ++msb) {
    n = L; m = msb;
    const long long cap = am_cap(L, msb);
    CHECK(cap == (long long)L * msb);
    if (L > 0 && msb > 0) CHECK((long long)(L - 1) * msb + msb - 1 == cap - 1);
    const int wcap = am_word_cap((int)cap);
    int words = 0;
    for (int p = 0; p < cap; p += 2) ++words;
    CHECK(words == wcap);
  }
  CHECK(am_cap(1 << 20, 4096) == (1LL << 32));
  // chunks of a block prefix sum cover [0, n) once
  for (n = 0; n <= 1100; ++n) {
    int covered = 0;
    for (int c = 0; c < am_chunks(n); ++c) for (int t = 0; t < AM_THREADS; ++t) covered += (c * AM_THREADS + t < n);
    CHECK(covered == n);
    CHECK(n == 0 || (am_chunks(n) - 1) * AM_THREADS < n);
  }
  // clamps and 64-bit offsets
  CHECK(am_clamp(-5, 0, 7) == 0 && am_clamp(9, 0, 7) == 7 && am_clamp(3, 0, 7) == 3 && am_clamp(1LL << 40, 0, 7) == 7 && am_clamp(-(1LL << 40), 0, 7) == 0);
  CHECK(am_clamp(4, 0, 0) == 0);
  {
    const int T = 3000, B = 1000, V = 1000;
    CHECK(am_lprobs_off(T - 1, B - 1, V - 1, B, V) == (long long)T * B * V - 1 && am_lprobs_off(T - 1, B - 1, V - 1, B, V) > (1LL << 31));
    CHECK(am_lprobs_off(0, 0, 0, B, V) == 0 && am_lprobs_off(1, 0, 0, B, V) == (long long)B * V && am_lprobs_off(0, 1, 0, B, V) == V);
    CHECK(am_row_off(69999, 69999, 70000) == 70000LL * 70000 - 1);
  }
  // the argmax order: sequential scan and a butterfly over 64 lanes agree with torch's rule
  {
    const float nan = std::nanf("");
    const float rows[4][3] = {{nan, 1, 2}, {1, 1, 0}, {0, nan, nan}, {-INFINITY, -INFINITY, -INFINITY}};
    const int want[4] = {0, 0, 1, 0};
    for (int r = 0; r < 4; ++r) {
      float bv[64]; int bi[64];
      for (int lane = 0; lane < 64; ++lane) {
        bv[lane] = -INFINITY; bi[lane] = 2147483647;
        for (int v = lane; v < 3; v += 64) if (am_argmax_wins(rows[r][v], v, bv[lane], bi[lane])) { bv[lane] = rows[r][v]; bi[lane] = v; }
      }
      for (int o = 32; o > 0; o >>= 1) {
        float nv[64]; int ni[64];
        for (int lane = 0; lane < 64; ++lane) {
          const bool w = am_argmax_wins(bv[lane ^ o], bi[lane ^ o], bv[lane], bi[lane]);
          nv[lane] = w ? bv[lane ^ o] : bv[lane]; ni[lane] = w ? bi[lane ^ o] : bi[lane];
        }
        for (int lane = 0; lane < 64; ++lane) { bv[lane] = nv[lane]; bi[lane] = ni[lane]; }
      }
      for (int lane = 0; lane < 64; ++lane) { n = r; i = lane; CHECK(bi[lane] == want[r]); }
    }
  }
  std::printf("OK %lld cells\n", cells);
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_index_header_sweep_on_the_host(tmp_path):
    src = tmp_path / "sweep.cpp"
    src.write_text(SWEEP)
    exe = tmp_path / "sweep"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "speecht5_amd", "csrc"), str(src),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


# ---- 4 ----
@pytest.mark.parametrize("mode", ["letter", "sentencepiece", None, "subword_nmt"])
def test_count_errors_host_against_the_reference(mode):
    syms = list("abcd") + ["|", "▁", "ab@@", "c@@", "▁ab", "é"]
    d = _Dictionary(syms, EXTRA)
    blank = d.index("<ctc_blank>")
    g = torch.Generator().manual_seed(11)
    T, B, V, L = 9, 6, len(d), 7
    lp = torch.log_softmax(torch.randn(T, B, V, generator=g) * 3, -1)
    lp[2, 1, :] = lp[2, 1, 4]          # a frame of ties
    lp[3, 2, 5] = float("nan")
    lens = torch.tensor([9, 0, 4, 12, -3, 7])
    target = torch.randint(0, V, (B, L), generator=g)
    target[0, 2], target[0, 4], target[5, :] = d.pad(), d.eos(), d.pad()
    got = A.count_errors_host(lp, lens, target, d, blank, mode)
    if mode == "subword_nmt":       # no table: the string form itself
        want = dict.fromkeys(A.KEYS, 0)
        for b in range(B):
            pred = R.greedy(lp[:, b].tolist(), int(lens[b]), blank)
            targ = [int(x) for x in target[b].tolist() if x not in (d.pad(), d.eos())]
            dist = R.levenshtein(post_process(d.string(pred), mode).split(), post_process(d.string(targ), mode).split())
            want["c_errors"] += R.levenshtein(pred, targ)
            want["c_total"] += len(targ)
            want["w_errors"] += dist
            want["wv_errors"] += dist
            want["w_total"] += len(post_process(d.string(targ), mode).split())
    else:
        want, _ = R.five_sums(lp.tolist(), lens.tolist(), target.tolist(), blank, d.pad(), d.eos(), table_of(d, mode))
    assert got == want
    assert all(isinstance(v, int) for v in got.values())


def test_count_errors_host_on_the_golden():
    for case in golden()["cases"]:
        d = _Dictionary(case["symbols"], EXTRA)
        got = A.count_errors_host(case["lprobs"], case["input_lengths"], case["target_label"], d, case["blank"], case["mode"])
        assert got == case["counts"], (case["mode"], got)


def test_strip_pad_eos_keeps_order():
    g = torch.Generator().manual_seed(5)
    t = torch.randint(0, 6, (9, 11), generator=g)
    t[3] = 1
    rows, lens = A.strip_pad_eos(t, 1, 2)
    assert rows.dtype == torch.int32 and lens.dtype == torch.int32
    for r, n, src in zip(rows.tolist(), lens.tolist(), t.tolist()):
        assert r[:n] == [x for x in src if x not in (1, 2)]


def test_a_tests_util_dictionary_is_enough_for_the_table():
    from tests.util import Dictionary
    d = Dictionary(5, EXTRA)      # list-like, no string()
    assert A.symbol_bytes(d, "letter")[:5] == [b"", b"<pad>", b"", b"<unk>", b"s0"]
    with pytest.raises(ValueError):
        A.symbol_bytes(d, "subword_nmt")


def test_gpu_wrappers_refuse_cpu_tensors():
    from speecht5_amd import functional as Fn
    with pytest.raises(TypeError):
        Fn.ctc_greedy_rows(torch.zeros(2, 1, 3), torch.tensor([2]), 0)
    with pytest.raises(TypeError):
        Fn.edit_distance_rows(torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                              torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        A.count_errors(torch.zeros(2, 1, 3), torch.tensor([2]), torch.zeros(1, 2, dtype=torch.long), _Dictionary(), 0)


# ---- 5 ----
def _suite(fault):
    """The checks of parts 1 and 2 with a fault planted in the reference: True when all of them still pass."""
    for case in golden()["cases"]:
        counts, rows = golden_counts(case, fault)
        if counts != case["counts"] or rows != case["rows"]:
            return False
    rng = random.Random(3)
    for a, b in _pairs(rng, 300, 14, 3):
        if R.levenshtein_diagonals(a, b, fault) != R.levenshtein(a, b):
            return False
    return True


def test_the_suite_passes_without_a_fault():
    assert _suite(None)


@pytest.mark.parametrize("fault", ["blank_first", "last_tie", "keep_eos", "hi_off", "sub_equal"])
def test_planted_faults_are_caught(fault):
    if fault == "hi_off":       # the missing cell is read as None: an error is a catch too
        try:
            assert not _suite(fault)
        except TypeError:
            pass
    else:
        assert not _suite(fault)


@pytest.mark.parametrize("fault,case_index", [("blank_first", 0), ("last_tie", 0), ("keep_eos", 0)])
def test_decoding_faults_are_caught_by_the_golden_alone(fault, case_index):
    case = golden()["cases"][case_index]
    counts, _ = golden_counts(case, fault)
    assert counts != case["counts"]


# ---- 6 ----
def test_kernels_keep_lds_in_ds_instructions_and_use_no_scratch():
    import importlib.util
    import re
    import tempfile
    spec = importlib.util.spec_from_file_location("barrier_audit", os.path.join(ROOT, "tools", "barrier_audit.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = os.path.join(tempfile.mkdtemp(), "asr_metrics.s")
    subprocess.check_call([m.HIPCC] + m.FLAGS + ["-o", out, os.path.join(ROOT, "speecht5_amd", "csrc", "asr_metrics.hip")],
                          stderr=subprocess.DEVNULL)
    assert not m.audit(out)
    bad, name, kernels = [], None, set()
    for line in open(out, errors="replace"):
        k = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if k and not k.group(1).startswith(".L"):
            name = k.group(1)
        elif name and re.match(r"^\s*(flat_|scratch_|buffer_atomic|global_atomic|ds_\w*(add|cmpst|max|min)_)", line):
            bad.append((name, line.strip()))
        elif name and re.match(r"^\s*s_barrier", line):
            kernels.add(name)
    assert not bad, bad
    assert any("edit_distance_kernel" in n for n in kernels)
