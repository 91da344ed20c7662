"""Batched text-to-waveform synthesis on the HIP kernels: csrc/ragged.hip, SpeechT5HifiGan.forward_ragged, Postnet.forward_ragged,
T5TransformerModel.synthesize_batch.

1. the ragged kernels against torch restatements, bit for bit, under poisoned allocations;
2. forward_ragged rows against forward(mel_b) per row, and against the HF golden;  3. no leak between rows;  4. chunking;
5. the ragged post-net against Postnet.forward per row;  6. synthesize_batch end to end (fp32: the batched decode is compared with the
   single-row decode at 1e-5, which only fp32 meets; the bf16 vocoder and post-net are covered by 2 - 5).

Bars of a packed row against its single-row call (`_row_bar`): fp32 1e-5 of the row's scale, the bar tests/test_tts_batch_gpu.py
holds a batched row to.  bf16: bit-equal.  That held in every case measured (profiles/tts_wave_parity.txt), so it is asserted; were
st5_gemm ever to pick another kernel or split for the packed M, the bar to fall back on is max |ragged - single| <= 2 * max |single -
fp64 restatement| per row (tests/hifigan_ragged_reference.py has the restatement)."""
import os

import pytest
import torch

from tests import hifigan_ragged_reference as R
from tests.util import G, build_tiny, close, load_golden, poisoned_allocations

pytestmark = pytest.mark.gpu

LENGTHS = [37, 5, 48, 1, 20]
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


def _row_bar(got, single, dtype, what):
    assert got.shape == single.shape, (what, got.shape, single.shape)
    assert bool(torch.isfinite(got).all()), what
    if dtype == torch.float32:
        close(got, single, 1e-5, what=what)
    else:
        assert torch.equal(got, single), f"{what}: bf16 max |ragged - single| {float((got - single).abs().max()):.3e}"


def _vocoder(cuda, size, dtype):
    from speecht5_amd import functional as Fn
    from speecht5_amd.hifigan import SpeechT5HifiGan
    Fn.set_compute_dtype(dtype)
    if size == "tiny":
        fx = torch.load(os.path.join(G, "tiny_hifigan.pt"), weights_only=False)
        m, cfg = SpeechT5HifiGan(**fx["config"]).eval(), dict(fx["config"])
        m.load_state_dict(fx["state_dict"])
    else:
        m, cfg = R.seeded_vocoder()
    return m.to(cuda), cfg, {k: v.detach().cpu() for k, v in m.state_dict().items()}


# ------------------------------------------------------------------------------------------------------------------------------
# 1. kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _act(x, act):
    from speecht5_amd import hip
    if act == hip.ACT_NONE:
        return x
    slope = 0.1 if act == hip.ACT_LRELU_01 else 0.01
    f = x.float()
    return torch.where(f > 0, f, f * torch.tensor(slope, dtype=torch.float32, device=x.device)).to(x.dtype)


@DTYPES
@pytest.mark.parametrize("rate", [1, 64])
@pytest.mark.parametrize("C", [32, 80, 256, 512])
def test_ragged_kernels_match_restatements_bit_for_bit(cuda, C, rate, dtype):
    from speecht5_amd import hip, ragged
    lengths, gap = [1, 5, 3], 2                                     # a first row of length 1; the layout ends with a gap
    with poisoned_allocations():
        lay = ragged.PackedLayout(lengths, gap, [0, 10, 20], cuda)
        T = lay.T
        assert T == 15 and lay.valid.tolist() == [1, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0]
        rows = lay.valid.bool().repeat_interleave(rate)
        g = torch.Generator().manual_seed(100 * C + rate)
        x = torch.randn(T * rate, C, generator=g).to(dtype).to(cuda)
        x[~rows] = float("nan")                                     # whatever a producer left in a gap row must not reach the output
        x[(~rows).nonzero()[0]] = float("inf")
        for act, (pl, pr) in ((hip.ACT_NONE, (3, 3)), (hip.ACT_LRELU_01, (25, 25)), (hip.ACT_LRELU_001, (0, 2))):
            got = lay.pad_act(x.view(1, T * rate, C), rate, pl, pr, act)
            want = torch.zeros(pl + T * rate + pr, C, dtype=dtype, device=cuda)
            want[pl:pl + T * rate][rows] = _act(x[rows], act)
            assert got.shape == (1, pl + T * rate + pr, C)
            assert torch.equal(got[0].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), (act, pl, pr)
        # gap zeroing in place: a buffer with `halo` rows in front and behind, filled with a pattern
        halo = 5
        buf = (torch.arange((T * rate + 2 * halo) * C, device=cuda) % 251 + 1).to(dtype).view(T * rate + 2 * halo, C)
        before = buf.clone()
        lay.zero_gaps(buf, rate, C, row0=halo)
        inner = buf[halo:halo + T * rate]
        assert torch.equal(inner[rows], before[halo:halo + T * rate][rows]), "a valid row was written"
        assert torch.equal(buf[:halo], before[:halo]) and torch.equal(buf[halo + T * rate:], before[halo + T * rate:]), "halo written"
        assert (inner[~rows] == 0).all()
        # a list that names a valid frame and frames out of range: skipped, nothing but gap rows is ever written
        bad = torch.tensor([0, 4, -1, T, T + 3, 1], dtype=torch.int32, device=cuda)
        buf2 = before.clone()
        hip.check(hip.lib().st5_ragged_zero_gaps(buf2.data_ptr() + halo * C * buf2.element_size(), lay.valid.data_ptr(), bad.data_ptr(),
                                                 bad.numel(), T, rate, C, hip.dt(buf2), hip.stream()), "st5_ragged_zero_gaps")
        want2 = before.clone()
        want2[halo + rate:halo + 2 * rate] = 0                       # frame 1 is the only gap frame in the list
        assert torch.equal(buf2, want2)
        torch.cuda.synchronize()


@DTYPES
def test_pack_and_unpack_match_indexing(cuda, dtype):
    from speecht5_amd import ragged
    lengths, gap, stride = [1, 7, 4], 3, 9
    g = torch.Generator().manual_seed(2)
    src = torch.randn(3 * stride, 80, generator=g).to(cuda)
    with poisoned_allocations():
        lay = ragged.PackedLayout(lengths, gap, [b * stride for b in range(3)], cuda)
        packed = lay.pack_rows(src, dtype)
        want = torch.zeros(lay.T, 80, dtype=dtype, device=cuda)
        for b, (o, n) in enumerate(zip(lay.offsets, lengths)):
            want[o:o + n] = src[b * stride:b * stride + n].to(dtype)
        assert torch.equal(packed, want)
        w = 4                                                        # a packed "waveform" of 4 samples per mel frame
        wave = torch.randn(lay.T * w, generator=g).to(dtype).to(cuda)
        flat, rows = lay.unpack_rows(wave, w)
        assert flat.dtype == torch.float32
        for b, (o, n) in enumerate(zip(lay.offsets, lengths)):
            assert torch.equal(rows[b].reshape(-1), wave[o * w:(o + n) * w].float())


# ------------------------------------------------------------------------------------------------------------------------------
# 2. rows equal single-row calls
# ------------------------------------------------------------------------------------------------------------------------------
def _b32_lengths():
    return torch.randint(20, 201, (32,), generator=torch.Generator().manual_seed(32)).tolist()


@DTYPES
@pytest.mark.parametrize("size,case", [("tiny", "five"), ("full", "five"), ("full", "b32")])
def test_forward_ragged_rows_equal_single_row_calls(cuda, size, case, dtype):
    m, _, _ = _vocoder(cuda, size, dtype)
    lengths = LENGTHS if case == "five" else _b32_lengths()
    mels = R.seeded_mels(lengths, seed=7)
    dev = [x.to(cuda) for x in mels]
    with poisoned_allocations():
        got = m.forward_ragged(dev)
    hop = m._packed_rate()
    assert len(got) == len(mels)
    for b, x in enumerate(dev):
        single = m(x)
        assert got[b].dtype == torch.float32 and got[b].shape == (hop * lengths[b],)
        _row_bar(got[b], single, dtype, f"{size} {case} row {b} (L {lengths[b]})")
    # the padded input form gives the same rows
    if case == "five":
        padded = torch.zeros(len(mels), max(lengths), 80, device=cuda)
        for b, x in enumerate(dev):
            padded[b, :lengths[b]] = x
        again = m.forward_ragged(padded, lengths=lengths)
        for a, b in zip(again, got):
            assert torch.equal(a, b)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 5e-2)], ids=["fp32", "bf16"])
def test_forward_ragged_meets_the_hf_golden_bars(cuda, dtype, tol):
    m, _, _ = _vocoder(cuda, "tiny", dtype)
    fx = torch.load(os.path.join(G, "tiny_hifigan.pt"), weights_only=False)
    spec = fx["spectrogram"]
    got = m.forward_ragged([spec[0].to(cuda), spec[1, :11].to(cuda), spec[1].to(cuda)])
    close(got[0], fx["waveform"][0], tol, what="golden row 0")
    close(got[2], fx["waveform"][1], tol, what="golden row 1")
    assert got[1].shape == (11 * m._packed_rate(),)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. no leak between rows
# ------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("size", ["tiny", "full"])
def test_other_rows_content_does_not_reach_a_row(cuda, size, dtype):
    """Same lengths and order, so the same layout and the same launches: only a leak between rows can change a row's bits."""
    m, _, _ = _vocoder(cuda, size, dtype)
    mels = [x.to(cuda) for x in R.seeded_mels(LENGTHS, seed=7)]
    other = [(x * 3.0 + 1.0).to(cuda) for x in R.seeded_mels(LENGTHS, seed=99)]
    base = m.forward_ragged(mels)
    for keep in (0, 2, 3):
        mixed = [mels[b] if b == keep else other[b] for b in range(len(mels))]
        got = m.forward_ragged(mixed)
        assert torch.equal(got[keep], base[keep]), f"row {keep} changed with the content of the other rows"
        assert not torch.equal(got[(keep + 1) % 5], base[(keep + 1) % 5])


# ------------------------------------------------------------------------------------------------------------------------------
# 4. chunking
# ------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("size", ["tiny", "full"])
def test_chunked_rows_equal_single_row_calls(cuda, size, dtype):
    from speecht5_amd import ragged
    m, _, _ = _vocoder(cuda, size, dtype)
    lengths = [30, 10, 25, 200, 5, 5, 40]
    chunks = ragged.plan_chunks(lengths, m.ragged_gap(), 100)
    assert len(chunks) == 3 and chunks[1] == [3]                    # three chunks, the over-long row alone
    mels = R.seeded_mels(lengths, seed=17)
    dev = [x.to(cuda) for x in mels]
    got = m.forward_ragged(dev, max_frames=100)
    for b, x in enumerate(dev):
        _row_bar(got[b], m(x), dtype, f"{size} chunked row {b}")


# ------------------------------------------------------------------------------------------------------------------------------
# 5. post-net
# ------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_postnet_ragged_rows_equal_single_row_calls(cuda, dtype):
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(dtype)
    post = R.seeded_postnet().to(cuda)
    befores = R.seeded_mels(LENGTHS, seed=4)
    dev = [x.to(cuda) for x in befores]
    state = {k: v.clone() for k, v in post.state_dict().items()}
    with poisoned_allocations():
        got = post.forward_ragged(dev)
    for k, v in post.state_dict().items():
        assert torch.equal(v, state[k]), f"{k} changed"             # running statistics and num_batches_tracked included
    for b, x in enumerate(dev):
        single = post(Fn.to_compute(x.unsqueeze(0))).squeeze(0)
        _row_bar(got[b], single, dtype, f"post-net row {b}")
    chunked = post.forward_ragged(dev, max_frames=60)
    for b, x in enumerate(dev):
        single = post(Fn.to_compute(x.unsqueeze(0))).squeeze(0)
        _row_bar(chunked[b], single, dtype, f"post-net chunked row {b}")
    post.postnet[2][1].train()
    with pytest.raises(RuntimeError):
        post.forward_ragged(dev)
    for k, v in post.state_dict().items():
        assert torch.equal(v, state[k]), f"{k} changed by the refused call"


# ------------------------------------------------------------------------------------------------------------------------------
# 6. end to end
# ------------------------------------------------------------------------------------------------------------------------------
def _tiny_model(cuda):
    model, args = build_tiny(cuda, torch.float32)
    return model.eval(), args


def _check_rows(out, singles, vocoder):
    for b, (got, ref) in enumerate(zip(out, singles)):
        wav, mel, probs, attn = got
        assert mel.shape == ref[0].shape, (b, mel.shape, ref[0].shape)
        close(mel, ref[0], 1e-5, what=f"row {b} mel")
        close(probs, ref[1], 1e-5, what=f"row {b} probs")
        assert attn.shape == ref[2].shape
        close(attn, ref[2], 1e-5, what=f"row {b} attn")
        if vocoder is None:
            assert wav is None
        else:
            _row_bar(wav, vocoder(ref[0]), torch.float32, f"row {b} wav")


def test_synthesize_batch_rows_equal_single_row_pipeline(cuda):
    from speecht5_amd import functional as Fn
    from tests.test_tts_batch_gpu import _assert_margin, _pick_stop_shift, _singles
    m, fx = load_golden("tiny_t2s.pt")
    ni = fx["sample"]["net_input"]
    toks, spk, lens = ni["src_tokens"].to(cuda), ni["spkembs"].to(cuda), ni["src_lengths"].tolist()
    model, args = _tiny_model(cuda)
    vocoder, _, _ = _vocoder(cuda, "tiny", torch.float32)
    assert vocoder.conv_pre.weight.shape[1] == model.speech_decoder_postnet.odim
    maxlen = [int(n * 20.0 / args.reduction_factor) for n in lens]
    shift, stops = _pick_stop_shift(_singles(model, toks, spk, lens), args.reduction_factor, maxlen)
    with torch.no_grad():
        model.speech_decoder_postnet.prob_out.bias.add_(shift)
    Fn.weight_cache.clear()
    singles = _singles(model, toks, spk, lens)
    for b, s in enumerate(singles):
        _assert_margin(s[1], 0.5, f"row {b}")
    out = model.synthesize_batch(src_tokens=toks, spkembs=spk, vocoder=vocoder, need_attn=True)
    steps = [o[1].shape[0] // args.reduction_factor for o in out]
    print(f"stop-logit shift {shift:+.4f}: steps {steps}")
    assert steps == stops and len(set(steps)) >= 2
    _check_rows(out, singles, vocoder)
    for o in out:
        assert o[0].shape == (o[1].shape[0] * vocoder._packed_rate(),)
    # chunked: each row in a chunk of its own gives the same rows
    tight = model.synthesize_batch(src_tokens=toks, spkembs=spk, vocoder=vocoder, need_attn=True, max_frames=1)
    _check_rows(tight, singles, vocoder)
    # no vocoder: wav is None, the same mel; no attention record by default
    bare = model.synthesize_batch(src_tokens=toks, spkembs=spk)
    for o, ref in zip(bare, out):
        assert o[0] is None and o[3] is None
        close(o[1], ref[1], 1e-5, what="mel without a vocoder")
        assert torch.equal(o[2], ref[2])
    # the batch entry point that exists stays what it was: generate_speech_batch rows against the same single rows
    for got, ref in zip(model.generate_speech_batch(src_tokens=toks, spkembs=spk), singles):
        close(got[0], ref[0], 1e-5, what="generate_speech_batch mel")


def test_synthesize_batch_speech_rows(cuda):
    m, fx = load_golden("tiny_t2s.pt")
    spk = fx["sample"]["net_input"]["spkembs"].to(cuda)
    model, _ = _tiny_model(cuda)
    vocoder, _, _ = _vocoder(cuda, "tiny", torch.float32)
    g = torch.Generator().manual_seed(55)
    n = [16000, 40000, 27200]
    src = torch.zeros(3, max(n))
    pad = torch.ones(3, max(n), dtype=torch.bool)
    for b, k in enumerate(n):
        src[b, :k] = torch.randn(k, generator=g) * 0.1
        pad[b, :k] = False
    src, pad = src.to(cuda), pad.to(cuda)
    out = model.synthesize_batch(source=src, spkembs=spk, padding_mask=pad, vocoder=vocoder, need_attn=True)
    singles = [model.generate_speech(source=src[b:b + 1, :k], spkembs=spk[b:b + 1],
                                     padding_mask=torch.zeros(1, k, dtype=torch.bool, device=cuda)) for b, k in enumerate(n)]
    _check_rows(out, singles, vocoder)


def test_task_synthesize_batch(cuda):
    from speecht5_amd.collate import TextToSpeechCollater
    from speecht5_amd.task import SpeechT5Task
    m, fx = load_golden("tiny_t2s.pt")
    ni = fx["sample"]["net_input"]
    toks, spk, lens = ni["src_tokens"], ni["spkembs"], ni["src_lengths"].tolist()
    model, args = _tiny_model(cuda)
    vocoder, _, _ = _vocoder(cuda, "tiny", torch.float32)
    task = SpeechT5Task.synthetic(args)
    g = torch.Generator().manual_seed(9)
    samples = [{"id": b, "audio_name": f"u{b}", "source": [toks[b, :lens[b]].to(cuda)],
                "target": torch.randn(6 + 2 * b, 80, generator=g).to(cuda), "spkembs": spk[b].to(cuda)} for b in range(3)]
    batch = TextToSpeechCollater(cuda, pad_idx=1, reduction_factor=args.reduction_factor).collater(samples)
    got = task.synthesize_batch([model], batch["net_input"], vocoder=vocoder)
    want = model.synthesize_batch(src_tokens=batch["net_input"]["src_tokens"], spkembs=batch["net_input"]["spkembs"], vocoder=vocoder)
    for a, b in zip(got, want):
        assert a[3] is None and b[3] is None
        for x, y in zip(a[:3], b[:3]):
            assert torch.equal(x, y)
