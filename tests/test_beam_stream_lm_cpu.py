"""Transformer-LM shallow fusion in the beam-search stream (speecht5_amd/beam_stream.py, st5_beam_lm_logprobs_sents of csrc/beam_lm.hip)
without a GPU:
1. what the per-slot LM kernel takes from csrc/beam_stream_index.h, compiled with the host compiler into a stand-alone program and
   swept against a Python restatement: the gate bst_slot_live over done in {0, 1}, pos from -1 to cap + 2 and a raw maxlen from -1 to
   cap + 1 (clamped by bst_maxlen, as the kernel clamps it), its old name bst_ctc_live, and the slot of a row for beams 1 to 32;
2. beam_stream.check_arguments with an LM: an LM that is not a TransformerLanguageModel, one with a larger dictionary than the
   model's and one with fewer positions than cap + 2 each raise a ValueError naming lm_model; a fitting LM passes, with and without
   joint_ctc."""
import os
import shutil
import subprocess
from argparse import Namespace

import pytest
import torch

from tests.util import Task, build_tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, N_SLOTS = 4, 3

# prints one line per case: "G done pos maxlen live alias" and "S beam row slot row0"
SWEEP = r"""
#include <cstdio>
#include "beam_stream_index.h"
int main() {
  const int cap = %d, n_slots = %d;
  for (int done = 0; done <= 1; ++done) for (int pos = -1; pos <= cap + 2; ++pos) for (int ml = -1; ml <= cap + 1; ++ml) {
    const int m = bst_maxlen(ml, cap);
    std::printf("G %%d %%d %%d %%d %%d\n", done, pos, ml, (int)bst_slot_live(done, pos, m), (int)bst_ctc_live(done, pos, m));
  }
  for (int beam = 1; beam <= 32; ++beam) for (long long row = 0; row < (long long)n_slots * beam; ++row)
    std::printf("S %%d %%lld %%lld %%lld\n", beam, row, bst_slot_of(row, beam), bst_row0(bst_slot_of(row, beam), beam));
  // a position or a row past 2^31 (the arguments are long long: nothing wraps)
  std::printf("X %%d %%lld\n", (int)bst_slot_live(0, 2147483648LL, 4), bst_slot_of(3LL * 2147483648LL + 5, 3));
  return 0;
}
""" % (CAP, N_SLOTS)


def _live(done, pos, maxlen, cap):
    """The restatement: the slot is not done and its step is one the beam step runs, under the limit brought into [0, cap]."""
    limit = min(max(maxlen, 0), cap)
    return int(done == 0 and 0 <= pos <= limit)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_gate_and_slot_of_a_row_on_the_host(tmp_path):
    src = tmp_path / "sweep.cpp"
    src.write_text(SWEEP)
    exe = tmp_path / "sweep"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "speecht5_amd", "csrc"), str(src),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    gates, slots, big = [], [], None
    for line in r.stdout.split("\n"):
        f = line.split()
        if f and f[0] == "G":
            gates.append(tuple(int(v) for v in f[1:]))
        elif f and f[0] == "S":
            slots.append(tuple(int(v) for v in f[1:]))
        elif f and f[0] == "X":
            big = (int(f[1]), int(f[2]))
    assert len(gates) == 2 * (CAP + 4) * (CAP + 3) and len(slots) == sum(N_SLOTS * b for b in range(1, 33))
    for done, pos, ml, live, alias in gates:
        assert live == alias == _live(done, pos, ml, CAP), (done, pos, ml, live, alias)
        if live:
            assert 0 <= pos <= CAP, "a live step is a column of tok below Tmax = cap + 2"
    assert sum(g[3] for g in gates) > 0 and not any(g[3] for g in gates if g[0] == 1)
    for beam, row, slot, row0 in slots:
        assert slot == row // beam and 0 <= slot < N_SLOTS and row0 == slot * beam and row0 <= row < row0 + beam, (beam, row, slot)
    assert big == (0, 2147483648 + 1)


# ---- the argument checks ----
@pytest.fixture(scope="module")
def tiny():
    model, _ = build_tiny(torch.device("cpu"), torch.float32)
    model.eval()
    return model, Task().dicts["text"]


def _lm(vocab, **kw):
    from speecht5_amd.transformer_lm import TransformerLanguageModel
    dims = dict(decoder_embed_dim=128, decoder_attention_heads=2, decoder_layers=1, decoder_ffn_embed_dim=128)
    return TransformerLanguageModel(Namespace(**dims, **kw), vocab=vocab, pad=1)


def test_check_arguments_with_an_lm(tiny):
    from speecht5_amd.beam_stream import check_arguments
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, d = tiny
    ok = dict(sentences=3, max_src_len=7000, decode="graph")
    ctc = dict(ctc_weight=0.4, ctc_rows=True)
    S, cap = check_arguments(SequenceGenerator([model], d, beam_size=2, max_len_b=20), **ok)
    assert cap == 20
    # a fitting LM passes, with and without joint_ctc: a smaller dictionary, and exactly cap + 2 positions
    for lm in (_lm(len(d) - 2), _lm(len(d)), _lm(len(d) - 2, tokens_per_sample=cap + 2)):
        assert check_arguments(SequenceGenerator([model], d, beam_size=2, max_len_b=20, lm_model=lm, lm_weight=0.5), **ok) == (S, cap)
        assert check_arguments(SequenceGenerator([model], d, beam_size=2, max_len_b=20, lm_model=lm, lm_weight=0.5, **ctc),
                               joint_ctc=True, **ok) == (S, cap)
    # each refusal names lm_model, with and without joint_ctc
    short = _lm(len(d) - 2, tokens_per_sample=cap + 1)
    assert short.max_positions() == cap + 1
    for lm, word in ((torch.nn.Identity(), "lm_model.*Identity"), (_lm(len(d) + 1), "lm_model.*dictionary"), (short, "lm_model.*positions")):
        with pytest.raises(ValueError, match=word):
            check_arguments(SequenceGenerator([model], d, beam_size=2, max_len_b=20, lm_model=lm), **ok)
        with pytest.raises(ValueError, match=word):
            check_arguments(SequenceGenerator([model], d, beam_size=2, max_len_b=20, lm_model=lm, **ctc), joint_ctc=True, **ok)
    # the limit that counts is the step limit at max_src_len, not the generator's max_len_b alone: a shorter stream fits the short LM
    assert check_arguments(SequenceGenerator([model], d, beam_size=2, max_len_b=cap - 1, lm_model=short), **ok) == (S, cap - 1)
    # the CTC keyword stays as it is with an LM
    with pytest.raises(ValueError, match="ctc_weight.*joint_ctc"):
        check_arguments(SequenceGenerator([model], d, beam_size=2, max_len_b=20, lm_model=_lm(len(d) - 2), **ctc), **ok)
