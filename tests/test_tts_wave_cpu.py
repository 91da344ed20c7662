"""The packed ("ragged") text-to-waveform path without a GPU: the gap rule, pinned from both sides in fp64
(tests/hifigan_ragged_reference.py), the function that computes the gap from the modules, and the chunk planner."""
import os

import pytest
import torch

from tests import hifigan_ragged_reference as R
from tests.util import G

LENGTHS = [37, 5, 48, 1, 20]


def _tiny():
    fx = torch.load(os.path.join(G, "tiny_hifigan.pt"), weights_only=False)
    return fx["state_dict"], dict(fx["config"])


def _worst(rows, singles):
    return max(float((a - b).abs().max()) for a, b in zip(rows, singles))


def test_gap_function_reads_the_modules():
    from speecht5_amd import ragged
    from speecht5_amd.hifigan import SpeechT5HifiGan
    full, cfg = R.seeded_vocoder()
    assert ragged.hifigan_gap(full) == R.gap_from_config(cfg) == 7          # kernel 11, dilation 5 at rate 4: ceil(25 / 4)
    assert ragged.postnet_gap(R.seeded_postnet(n_chans=8)) == 2             # kernel 5 at rate 1
    _, tcfg = _tiny()
    # tiny golden: rates 4, 4; resblock kernels 3, 7; dilations 1, 3, 5.  Pads at rate 4: 1, 3, 5 (k 3) and 3, 9, 15 (k 7) ->
    # ceil(15 / 4) = 4; at rate 16 at most ceil(15 / 16) = 1; conv_pre and conv_post kernel 7 -> 3 at rate 1, 1 at rate 16.
    assert ragged.hifigan_gap(SpeechT5HifiGan(**tcfg)) == R.gap_from_config(tcfg) == 4
    assert ragged.halo_gap([(25, 4), (3, 1)]) == 7 and ragged.halo_gap([(2, 1)]) == 2 and ragged.halo_gap([(1, 16)]) == 1


@pytest.mark.parametrize("size", ["tiny", "full"])
def test_packed_rows_equal_single_rows_in_fp64_with_the_gap_of_the_rule(size):
    if size == "tiny":
        sd, cfg = _tiny()
    else:
        m, cfg = R.seeded_vocoder()
        sd = m.state_dict()
    mels = R.seeded_mels(LENGTHS, seed=3)
    gap = R.gap_from_config(cfg)
    with torch.no_grad():
        singles = [R.hifigan_single(sd, cfg, m) for m in mels]
        rows = R.hifigan_packed(sd, cfg, mels, gap)
        for a, b in zip(rows, singles):
            assert a.shape == b.shape
        err = _worst(rows, singles)
        print(f"{size}: gap {gap}: worst row differs by {err:.2e}")
        assert err <= 1e-12
        if size == "full":
            short = _worst(R.hifigan_packed(sd, cfg, mels, gap - 1), singles)
            unzeroed = _worst(R.hifigan_packed(sd, cfg, mels, gap, zero=False), singles)
            print(f"full: gap {gap - 1}: {short:.2e}; gap {gap}, nothing zeroed: {unzeroed:.2e}")
            assert short > 1e-4
            assert unzeroed > 1e-4


def test_packed_postnet_rows_equal_single_rows_in_fp64():
    layers = R.postnet_layers(R.seeded_postnet())
    befores = R.seeded_mels(LENGTHS, seed=4)
    with torch.no_grad():
        singles = [R.postnet_single(layers, m) for m in befores]
        for gap in (2, 7):
            assert _worst(R.postnet_packed(layers, befores, gap), singles) <= 1e-12
        assert _worst(R.postnet_packed(layers, befores, 1), singles) > 1e-4
        assert _worst(R.postnet_packed(layers, befores, 7, zero=False), singles) > 1e-4


def test_chunk_planner():
    from speecht5_amd.ragged import plan_chunks
    lengths, gap = [30, 10, 25, 200, 5, 5, 40], 7
    chunks = plan_chunks(lengths, gap, 100)
    assert [b for c in chunks for b in c] == list(range(len(lengths)))       # order kept, every row exactly once
    assert chunks == [[0, 1, 2], [3], [4, 5, 6]]
    for c in chunks:
        assert sum(lengths[b] + gap for b in c) <= 100 or len(c) == 1         # cap respected; an over-long row alone
    assert plan_chunks(lengths, gap, None) == [list(range(len(lengths)))]
    assert plan_chunks([3, 3], 2, 1) == [[0], [1]]
    assert plan_chunks([37, 37, 37], 7, 88) == [[0, 1], [2]]
    with pytest.raises(ValueError):
        plan_chunks([4, 0], 2, 100)


def test_layout_tables():
    from speecht5_amd.ragged import layout_tables
    offsets, T, pack, unpack, gaps = layout_tables([1, 3], 2, [10, 20])
    assert offsets == [0, 3] and T == 8
    assert pack.tolist() == [10, -1, -1, 20, 21, 22, -1, -1]
    assert unpack.tolist() == [0, 3, 4, 5] and gaps.tolist() == [1, 2, 6, 7]
