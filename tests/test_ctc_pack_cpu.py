"""The replayed ASR fine-tuning update, without a GPU:
1. tests/ctc_pack_reference.py (the numpy restatement of st5_ctc_pack_rows' contract) against torch's masked_select + cumsum form on
   random rows: the packed rows, read at offsets b * L with the kept counts, ARE the flat targets the criterion builds today.
2. tools/ctc_pack_sweep.cpp: csrc/ctc_pack_index.h walked on the host as the kernel walks it, built with the address and
   undefined-behaviour sanitizers and run directly; two planted faults must be caught by the same sweep.
3. header / binding agreement of the new symbol.
4. the feed audit: graph.HOST_VALUES_FREE["s2t"], train_stats.check_feed_host_values with and without the criterion's options, and
   update.check_s2t_source's refusals by name.
5. collate.SpeechToTextCollater.plan / host_padding_mask: the fixed shape, its refusals, the mirror.
6. update.freeze_thresholds / freeze_crossing: which replay crosses a freeze boundary."""
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.ctc_pack_reference import pack_rows, rows_of_every_kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, EOS = 1, 2


# ---- 1 ----
@pytest.mark.parametrize("B,L", [(1, 1), (3, 7), (5, 64), (4, 65), (2, 257), (7, 600), (6, 130)])
def test_restatement_equals_masked_select_and_cumsum(B, L):
    t = rows_of_every_kind(B, L, PAD, EOS, 40, seed=B * 1000 + L)
    packed, offsets, kept, total = pack_rows(t, PAD, EOS)
    tt = torch.from_numpy(t)
    mask = (tt != PAD) & (tt != EOS)
    flat = tt.masked_select(mask)
    lengths = mask.sum(-1)
    starts = torch.cumsum(lengths, 0) - lengths
    assert kept.tolist() == lengths.tolist() and int(total[0]) == flat.numel() and offsets.tolist() == [b * L for b in range(B)]
    for b in range(B):
        n = int(lengths[b])
        assert packed[b, :n].tolist() == flat[int(starts[b]):int(starts[b]) + n].tolist()
        assert (packed[b, n:] == PAD).all()
    # what the CTC kernels read: targets[offsets[b] + i] for i < length_b
    read = np.concatenate([packed.reshape(-1)[offsets[b]:offsets[b] + kept[b]] for b in range(B)]) if B else np.zeros(0)
    assert read.tolist() == flat.tolist()


def test_collater_rows_give_target_lengths_minus_one():
    """The precondition: labels hold neither pad nor eos -> kept == target_lengths - 1 (the criterion's lengths)."""
    rng = np.random.RandomState(3)
    n = [0, 5, 8, 3]
    L = max(n) + 1
    t = np.full((4, L), PAD, dtype=np.int64)
    for b, k in enumerate(n):
        t[b, :k] = rng.randint(4, 30, size=k)
        t[b, k] = EOS
    _, _, kept, total = pack_rows(t, PAD, EOS)
    assert kept.tolist() == n and int(total[0]) == sum(n)


# ---- 2 ----
def _sweep(tmp_path, *defines):
    exe = tmp_path / ("sweep" + "".join(defines).replace("-D", "_"))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *defines, "-I", os.path.join(ROOT, "speecht5_amd", "csrc"), os.path.join(ROOT, "tools", "ctc_pack_sweep.cpp"),
                           "-o", str(exe)])
    return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_index_header_sweep_on_the_host(tmp_path):
    r = _sweep(tmp_path)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
@pytest.mark.parametrize("fault", ["PLANT_INCLUSIVE", "PLANT_TAIL_FROM_CHUNK"])
def test_index_header_sweep_catches_planted_faults(tmp_path, fault):
    r = _sweep(tmp_path, "-D" + fault)
    assert r.returncode == 1 and "FAILED" in r.stdout, (fault, r.stdout + r.stderr)


# ---- 3 ----
def test_header_and_binding_agree():
    from ctypes import c_int, c_int32, c_int64, c_void_p
    from speecht5_amd import hip
    assert "st5_ctc_pack_rows" in hip.exported_symbols()
    hdr = open(os.path.join(ROOT, "include", "speecht5_hip.h")).read()
    decl = re.search(r"int st5_ctc_pack_rows\(([^;]*)\);", hdr).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["const int64_t* target", "int64_t pad", "int64_t eos", "int32_t B", "int32_t L", "int64_t* packed", "int64_t* offsets",
                    "int64_t* kept", "int64_t* total", "void* stream"]
    ctype = {"int64_t": c_int64, "int32_t": c_int32}
    want = [c_void_p if "*" in a else ctype[a.split()[0]] for a in args]
    res, sig = hip._SIGS["st5_ctc_pack_rows"]
    assert res is c_int and sig == want
    src = open(os.path.join(ROOT, "speecht5_amd", "csrc", "ctc_loss.hip")).read()
    assert re.search(r'extern "C" int st5_ctc_pack_rows\(', src) and '#include "ctc_pack_index.h"' in src


# ---- 4 ----
def _crit(**kw):
    return SimpleNamespace(**{"sentence_avg": True, "ctc_weight": 0.5, "device_targets": True, **kw})


def test_s2t_free_values_and_the_stats_audit():
    from speecht5_amd.graph import HOST_VALUES_FREE
    from speecht5_amd.train_stats import LOGGED_SAMPLE_VALUES, check_feed_host_values, device_logged
    assert HOST_VALUES_FREE["s2t"] == ("ntokens", "nsentences")
    assert HOST_VALUES_FREE["speech_pretrain"] == ("ntokens", "ntokens_list", "nsentences", "src_lengths")
    assert HOST_VALUES_FREE["text_pretrain"] == ("nsentences",)
    assert LOGGED_SAMPLE_VALUES["s2t"] == {"ntokens": "ntokens", "sample_size": "ntokens"}       # (the table's entries are kept)
    # without the options the audit refuses s2t under a source, by name
    with pytest.raises(ValueError, match="s2t.*ntokens"):
        check_feed_host_values(["s2t"], HOST_VALUES_FREE)
    # exactly device_targets=True takes `ntokens` off the host; sentence_avg=True makes sample_size B
    assert device_logged("s2t", _crit()) == ("ntokens", "sample_size")
    assert device_logged("s2t", _crit(device_targets=False)) == ("sample_size",)
    assert device_logged("s2t", SimpleNamespace(text_criterion=_crit())) == ("ntokens", "sample_size")      # (SpeechT5Criterion's part)
    assert device_logged("text_pretrain", _crit()) == ()
    check_feed_host_values(["s2t"], HOST_VALUES_FREE, {"s2t": device_logged("s2t", _crit())})
    with pytest.raises(ValueError, match="s2t.*`ntokens`"):
        check_feed_host_values(["s2t"], HOST_VALUES_FREE, {"s2t": device_logged("s2t", _crit(device_targets=False))})
    with pytest.raises(ValueError, match="s2t.*`sample_size`"):
        check_feed_host_values(["s2t"], HOST_VALUES_FREE, {"s2t": device_logged("s2t", _crit(sentence_avg=False))})
    # no other task's host value can be declared away
    with pytest.raises(ValueError, match="text_pretrain"):
        check_feed_host_values(["text_pretrain"], HOST_VALUES_FREE, {"text_pretrain": ("ntokens",)})
    # the other fine-tuning tasks stay refused under a source: their free list is empty and their ntokens is logged from the host
    for name in ("t2s", "s2s", "s2c"):
        assert name not in HOST_VALUES_FREE
        with pytest.raises(ValueError, match=name):
            check_feed_host_values([name], dict(HOST_VALUES_FREE, **{name: ("ntokens",)}))


def test_update_refuses_an_s2t_source_by_option():
    from speecht5_amd.update import check_s2t_source
    mb = [{"task_name": "s2t"}]
    check_s2t_source(mb, _crit())
    check_s2t_source(mb, _crit(ctc_weight=0.0, device_targets=False))          # no CTC term: no masked_select
    check_s2t_source([{"task_name": "speech_pretrain"}], _crit(sentence_avg=False, device_targets=False))
    check_s2t_source(mb, _crit(sentence_avg=False), graph=False)               # an eager update runs every batch as it is
    with pytest.raises(ValueError, match="sentence_avg"):
        check_s2t_source(mb, _crit(sentence_avg=False))
    with pytest.raises(ValueError, match="device_targets"):
        check_s2t_source(mb, _crit(device_targets=False))
    with pytest.raises(ValueError, match=r"micro_batches\[1\].*device_targets"):
        check_s2t_source([{"task_name": "text_pretrain"}, {"task_name": "s2t"}], SimpleNamespace(text_criterion=_crit(device_targets=False)))


def test_criterion_keyword_is_keyword_only_and_off_by_default():
    import inspect
    from speecht5_amd.criterions import SpeechT5Criterion, SpeechtoTextLoss
    p = inspect.signature(SpeechtoTextLoss.__init__).parameters["device_targets"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert inspect.signature(SpeechT5Criterion.__init__).parameters["device_targets"].default is False


# ---- 5 ----
def test_fixed_shape_plan_and_refusals():
    from speecht5_amd.collate import SpeechToTextCollater as C
    assert C.plan([7, 8], [4000, 3000], [5, 9]) == (4000, 10)                  # the batch's own maxima: longest label + </s>
    assert C.plan([7, 8], [4000, 3000], [5, 9], (6000, 12)) == (6000, 12)
    assert C.plan([7, 8], [6000, 3000], [5, 11], (6000, 12)) == (6000, 12)     # exactly fitting
    with pytest.raises(ValueError, match=r"item 8.*6001 samples"):
        C.plan([7, 8], [4000, 6001], [5, 9], (6000, 12))
    with pytest.raises(ValueError, match=r"item 7.*12 labels"):
        C.plan([7, 8], [4000, 3000], [12, 9], (6000, 12))
    for bad in ((0, 4), (4,), (4.0, 4), "ab"):
        with pytest.raises(ValueError, match="fixed_shape"):
            C("cpu", fixed_shape=bad)
    assert C("cpu").fixed_shape is None and C("cpu", fixed_shape=[6000, 12]).fixed_shape == (6000, 12)


def test_host_mirror_is_arange_ge_length():
    from speecht5_amd.collate import SpeechToTextCollater as C
    from speecht5_amd.graph import padding_mirror
    sizes, S = [6000, 4200, 0, 1], 6000
    m = C.host_padding_mask(sizes, S)
    assert m.dtype == torch.bool and m.device.type == "cpu" and tuple(m.shape) == (4, S)
    assert torch.equal(m, torch.arange(S)[None, :] >= torch.tensor(sizes)[:, None])
    # the feed takes it as the batch's mirror (a sample without it and without host src_lengths is refused)
    pm = torch.zeros(4, S, dtype=torch.bool)
    with pytest.raises(ValueError, match="src_lengths"):
        padding_mirror({"net_input": {"padding_mask": pm}, "task_name": "s2t"})
    pm._st5_host = m
    assert padding_mirror({"net_input": {"padding_mask": pm}, "task_name": "s2t"}) is m


# ---- 6 ----
def test_freeze_crossing():
    from speecht5_amd.update import freeze_crossing, freeze_thresholds

    class M(torch.nn.Module):
        def __init__(self, **kw):
            super().__init__()
            for k, v in kw.items():
                setattr(self, k, v)

    model = torch.nn.Sequential(M(freeze_encoder_updates=4), M(freeze_encoder_updates=4, freeze_decoder_updates=0), M(other=3))
    thr = freeze_thresholds(model)
    assert thr == {"freeze_encoder_updates": [4], "freeze_decoder_updates": [0]}
    assert freeze_crossing(thr, 3, 3) is None and freeze_crossing(thr, 1, 3) is None
    assert freeze_crossing(thr, 3, 4) == ("freeze_encoder_updates", 4)         # update 4 is the first with 4 <= num_updates
    assert freeze_crossing(thr, 4, 400) is None and freeze_crossing(thr, 6, 3) == ("freeze_encoder_updates", 4)
    assert freeze_crossing({"freeze_decoder_updates": [0]}, 1, 10 ** 6) is None
