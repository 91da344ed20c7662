"""The three rules of the length-exact batched speech encoding, on the CPU in fp64 (tests/speech_rows_reference.py) with the
pre-net weights of the tiny golden model:

1. the restatement's single-clip form is the verbatim oracle's pre-net (1e-10);
2. the length-aware padded batch equals the single clips (1e-12) on 16000 / 40000 / 27200 / 400 / 16079 / 16080 samples;
3. the exact frame mask t >= T_b differs from the reference's chunk mask;
4. negative control: the reference's padded batch does NOT equal the single clips (by far more than 1e-6)."""
from types import SimpleNamespace

import pytest
import torch

from tests import speech_rows_reference as R
from tests.util import load_golden

GPU_LENGTHS = [16000, 40000, 27200]      # the rows of tests/test_speech_rows_gpu.py's negative control: margin checked below


@pytest.fixture(scope="module")
def tiny():
    m, _ = load_golden(None)
    cfg = SimpleNamespace(**m["args"])
    sd32 = {k: v.detach().clone() for k, v in m["state_dict"].items() if k.startswith(R.PRE)}
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
    return SimpleNamespace(cfg=cfg, sd=sd, layers=R.layers_of(cfg))


def test_recipe_frame_arithmetic(tiny):
    assert [R.frames(n, tiny.layers) for n in R.LENGTHS] == [49, 124, 84, 1, 49, 50]
    assert R.frames(399, tiny.layers) == 0


def test_single_clip_form_is_the_oracles_prenet(tiny, monkeypatch):
    """The oracle casts to fp32 in two places (`x.float()` before GroupNorm, the feature penalty); with Tensor.float the identity for
    the duration of the call the verbatim oracle code runs in fp64 on the fp64 weights, and the restatement must match it to
    round-off.  (In fp32 the two agree to ~1e-6, which would pin nothing at the 1e-12 the batch comparison works at.)"""
    from oracle import speecht5_oracle as O
    _, _, clips = R.padded_batch([16079], seed=3)
    want_x, want_m = R.single(tiny.sd, tiny.cfg, clips[0])
    monkeypatch.setattr(torch.Tensor, "float", lambda self, *a, **k: self)
    with torch.no_grad():
        ref = O.speech_encoder_prenet(tiny.sd, tiny.cfg, clips[0][None, :], torch.zeros(1, clips[0].numel(), dtype=torch.bool))
    monkeypatch.undo()
    assert ref["x"].dtype == torch.float64
    assert torch.equal(ref["padding_mask"], want_m)
    err = R.rel_err(want_x, ref["x"])
    print(f"restatement vs oracle, one clip of 16079 samples: {err:.2e}")
    assert err <= 1e-10


def test_single_clip_form_tracks_the_oracle_in_fp32(tiny):
    """The same tie with nothing patched: the oracle as it is, fp32 weights and clip, against the fp64 restatement.  Bound: fp32
    unit round-off 6e-8 times the ~100 roundings that feed one output value (seven convolutions of up to 192 terms, three
    normalisations, the 16 x 32-term positional convolution), i.e. 1e-5 relative to the largest output."""
    from oracle import speecht5_oracle as O
    _, _, clips = R.padded_batch([16079], seed=3)
    want_x, want_m = R.single(tiny.sd, tiny.cfg, clips[0])
    m, _ = load_golden(None)
    sd32 = {k: v.detach().float() for k, v in m["state_dict"].items() if k.startswith(R.PRE)}
    with torch.no_grad():
        ref = O.speech_encoder_prenet(sd32, tiny.cfg, clips[0].float()[None, :], torch.zeros(1, clips[0].numel(), dtype=torch.bool))
    assert ref["x"].dtype == torch.float32 and torch.equal(ref["padding_mask"], want_m)
    err = R.rel_err(want_x, ref["x"].double())
    print(f"fp64 restatement vs the fp32 oracle, one clip of 16079 samples: {err:.2e}")
    assert err <= 1e-5


def test_aware_batch_equals_single_clips(tiny):
    wav, pad, clips = R.padded_batch(R.LENGTHS, seed=1)
    with torch.no_grad():
        x, pm = R.prenet(tiny.sd, tiny.cfg, wav, lens=R.LENGTHS)
        for b, n in enumerate(R.LENGTHS):
            xs, _ = R.single(tiny.sd, tiny.cfg, clips[b])
            T = xs.size(1)
            assert T == R.frames(n, tiny.layers)
            assert pm[b].tolist() == [False] * T + [True] * (x.size(1) - T)
            err = R.rel_err(x[b, :T], xs[0])
            print(f"row {b} ({n} samples, {T} frames): aware batch vs single {err:.2e}")
            assert err <= 1e-12


def test_aware_batch_ignores_what_the_padding_holds(tiny):
    with torch.no_grad():
        a, _ = R.prenet(tiny.sd, tiny.cfg, R.padded_batch(R.LENGTHS, seed=1)[0], lens=R.LENGTHS)
        b, _ = R.prenet(tiny.sd, tiny.cfg, R.padded_batch(R.LENGTHS, seed=1, fill=0.37)[0], lens=R.LENGTHS)
    for r, n in enumerate(R.LENGTHS):
        T = R.frames(n, tiny.layers)
        assert R.rel_err(a[r, :T], b[r, :T]) <= 1e-12


def test_exact_mask_differs_from_the_chunk_mask(tiny):
    _, pad, _ = R.padded_batch(R.LENGTHS)
    T = R.frames(max(R.LENGTHS), tiny.layers)
    chunk = R.chunk_mask(pad, T)
    exact = R.exact_mask(R.LENGTHS, T, tiny.layers)
    valid_chunk, valid_exact = (~chunk).sum(1).tolist(), (~exact).sum(1).tolist()
    print(f"valid frames: chunk rule {valid_chunk}, exact {valid_exact}")
    assert valid_exact == [49, 124, 84, 1, 49, 50]
    assert any(c != e for c, e in zip(valid_chunk, valid_exact))
    assert all(c >= e for c, e in zip(valid_chunk, valid_exact))      # the chunk rule never masks a frame the row owns


@pytest.mark.parametrize("lengths", [R.LENGTHS, GPU_LENGTHS], ids=["six", "gpu_rows"])
def test_negative_control_unaware_batch_differs(tiny, lengths):
    wav, pad, clips = R.padded_batch(lengths, seed=1)
    longest = lengths.index(max(lengths))
    with torch.no_grad():
        x, _ = R.prenet(tiny.sd, tiny.cfg, wav, padding_mask=pad)
        for b, n in enumerate(lengths):
            xs, _ = R.single(tiny.sd, tiny.cfg, clips[b])
            err = R.rel_err(x[b, :xs.size(1)], xs[0])
            print(f"row {b} ({n} samples): unaware batch vs single {err:.2e}")
            if b == longest:
                assert err <= 1e-12            # (the longest row has no padding: the reference form is exact for it)
            else:
                assert err > 1e-6
                if lengths is GPU_LENGTHS:
                    assert err > 1e-3          # the margin tests/test_speech_rows_gpu.py's negative control relies on
