"""Streaming synthesis (T5TransformerModel.generate_speech_stream / synthesize_stream, speecht5_amd/tts_stream.py) on the tiny golden
model: the stream against single-utterance generate_speech, its schedule against stream_schedule, invariance of a result under the
row, the admission tick and the neighbours (bit for bit), pre-net dropout, speech sources, the vocoder path, the refusals, and the
batch path before and after a stream."""
from types import SimpleNamespace

import pytest
import torch

from tests.test_tts_batch_gpu import _assert_margin, _pick_stop_shift
from tests.util import build_tiny, close, load_golden

pytestmark = pytest.mark.gpu

STEPS = [16, 4, 4, 4, 12, 4, 4, 8, 4]          # the anchor case of tests/test_tts_stream_cpu.py
ROWS, POLL = 3, 4


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


def _tiny(cuda, dtype=torch.float32):
    model, args = build_tiny(cuda, dtype)
    model.eval()
    model.TTS_POLL_STEPS = POLL                 # (on the instance, for the test)
    return model, args


@pytest.fixture(scope="module")
def golden():
    _, fx = load_golden("tiny_t2s.pt")
    ni = fx["sample"]["net_input"]
    return SimpleNamespace(toks=ni["src_tokens"], spk=ni["spkembs"], lens=ni["src_lengths"].tolist())


def _text(golden, i, n):
    """n tokens built from golden text i % 3 by repetition / truncation."""
    row = golden.toks[i % 3, :golden.lens[i % 3]]
    return row.repeat((n + row.numel() - 1) // row.numel())[:n].clone()


def _nine(golden, r, cuda):
    """Nine requests whose text lengths give, with threshold=2.0 (which also stands for both length ratios), exactly STEPS."""
    reqs = []
    for i, s in enumerate(STEPS):
        n = s * r // 2
        assert int(n * 2.0 / r) == s
        reqs.append((f"u{i}", _text(golden, i, n).to(cuda), golden.spk[i % 3].to(cuda)))
    return reqs


def _single(model, req, **kw):
    _, src, spk = req
    return model.generate_speech(src_tokens=src.unsqueeze(0), spkembs=spk.unsqueeze(0), **kw)


@pytest.fixture(scope="module")
def nine_singles(cuda, golden):
    """generate_speech of each of the nine requests alone (threshold 2.0), computed once and left unchanged."""
    model, args = _tiny(cuda)
    reqs = _nine(golden, args.reduction_factor, cuda)
    return [tuple(t.clone() for t in _single(model, q, threshold=2.0)) for q in reqs]


def _same_as_single(got, ref, what, tol=1e-5):
    _, mel, probs, attn = got
    assert mel.shape == ref[0].shape and probs.shape == ref[1].shape, (what, mel.shape, ref[0].shape)
    close(mel, ref[0], tol, what=f"{what} mel")
    close(probs, ref[1], tol, what=f"{what} probs")
    if attn is not None:
        assert attn.shape == ref[2].shape, (what, attn.shape, ref[2].shape)
        close(attn, ref[2], tol, what=f"{what} attn")


# ---- the stream equals the singles, and runs stream_schedule's schedule ----
@pytest.mark.parametrize("decode", ["device", "graph"])
def test_stream_equals_singles_and_follows_the_schedule(cuda, golden, nine_singles, decode):
    from speecht5_amd.tts_stream import stream_schedule
    model, args = _tiny(cuda)
    reqs = _nine(golden, args.reduction_factor, cuda)
    out = list(model.generate_speech_stream(iter(reqs), rows=ROWS, max_src_len=16 * args.reduction_factor // 2, decode=decode,
                                            need_attn=True, threshold=2.0))
    ticks, order = stream_schedule(STEPS, ROWS, POLL)
    assert (ticks, order) == (24, [1, 2, 3, 5, 0, 6, 4, 8, 7])
    assert [o[0] for o in out] == [f"u{i}" for i in order]
    assert model.tts_device_steps + model.tts_graph_replays == ticks
    assert (model.tts_graph_replays > 0) == (decode == "graph") and model.tts_decode_mode == decode
    for o in out:
        i = int(o[0][1:])
        assert o[1].shape[0] == STEPS[i] * args.reduction_factor
        _same_as_single(o, nine_singles[i], o[0])


def test_data_dependent_stops_match_singles(cuda, golden):
    from speecht5_amd import functional as Fn
    model, args = _tiny(cuda)
    r = args.reduction_factor
    reqs = [(f"g{k}", golden.toks[i, :golden.lens[i]].to(cuda), golden.spk[i].to(cuda)) for k, i in enumerate((0, 1, 2, 2, 0, 1))]
    maxlen = [int(golden.lens[i] * 20.0 / r) for i in range(3)]
    shift, stops = _pick_stop_shift([_single(model, q) for q in reqs[:3]], r, maxlen)
    with torch.no_grad():
        model.speech_decoder_postnet.prob_out.bias.add_(shift)
    Fn.weight_cache.clear()
    singles = [_single(model, q) for q in reqs[:3]]
    for b, s in enumerate(singles):
        _assert_margin(s[1], 0.5, f"text {b}")
    out = list(model.generate_speech_stream(reqs, rows=2, max_src_len=max(golden.lens), need_attn=True))
    assert sorted(o[0] for o in out) == sorted(q[0] for q in reqs), "no row may be left out of the comparison"
    by_key = {o[0]: o for o in out}
    lens = []
    for i, (key, _, _) in zip((0, 1, 2, 2, 0, 1), reqs):
        _same_as_single(by_key[key], singles[i], key)
        lens.append(by_key[key][1].shape[0] // r)
    print(f"stop-logit shift {shift:+.4f}: steps {lens} (predicted {stops}, maxlen {maxlen})")
    assert lens == [stops[i] for i in (0, 1, 2, 2, 0, 1)] and len(set(lens)) >= 2
    assert any(n < maxlen[i] for n, i in zip(lens, (0, 1, 2, 2, 0, 1)))


# ---- invariance: the race detector ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_result_does_not_depend_on_row_tick_or_neighbours(cuda, golden, dtype):
    model, args = _tiny(cuda, dtype)
    r = args.reduction_factor
    nine = _nine(golden, r, cuda)
    probe = lambda k: (k, nine[7][1], nine[7][2])        # noqa: E731  (8 steps)
    reqs = [probe("first")] + nine[:3] + [probe("middle")] + nine[3:6] + [probe("last")]
    res = {}
    for decode in ("device", "graph"):
        out = list(model.generate_speech_stream(reqs, rows=ROWS, max_src_len=16 * r // 2, decode=decode, need_attn=True, threshold=2.0))
        assert len(out) == len(reqs)
        res[decode] = {o[0]: o for o in out}
    a = res["device"]["first"]
    assert bool(torch.isfinite(a[1].float()).all()) and a[1].shape[0] == 8 * r
    for k in ("middle", "last"):
        for j in (1, 2, 3):
            assert torch.equal(res["device"][k][j], a[j]), (k, j)
    for key, o in res["device"].items():
        for j in (1, 2, 3):
            assert torch.equal(res["graph"][key][j], o[j]), f"graph != device for {key}[{j}]"


# ---- pre-net dropout ----
def test_prenet_dropout_draws_per_row_and_tick(cuda, golden):
    model, args = _tiny(cuda)
    q = _nine(golden, args.reduction_factor, cuda)[4]
    reqs = [("a", q[1], q[2]), ("b", q[1], q[2]), ("c", q[1], q[2])]
    kw = dict(rows=2, max_src_len=32, threshold=2.0)
    same = {o[0]: o for o in model.generate_speech_stream(reqs, **kw)}
    assert torch.equal(same["a"][1], same["b"][1]) and torch.equal(same["a"][1], same["c"][1])
    tac = model.speech_decoder_prenet.decoder_prenet[0][0]
    tac.dropout_rate = 0.5
    try:
        diff = {o[0]: o for o in model.generate_speech_stream(reqs, **kw)}
    finally:
        tac.dropout_rate = 0.0
    assert all(bool(torch.isfinite(o[1]).all()) for o in diff.values())
    assert diff["a"][1].shape == diff["b"][1].shape == same["a"][1].shape
    assert not torch.equal(diff["a"][1], diff["b"][1])          # two rows, the same ticks
    assert not torch.equal(diff["a"][1], diff["c"][1])          # the same row, later ticks


# ---- speech sources ----
def test_speech_sources_match_single_clip_calls(cuda, golden):
    model, _ = _tiny(cuda)
    g = torch.Generator().manual_seed(55)
    n = [4000, 8000, 6000]
    reqs = [(f"clip{b}", (torch.randn(m, generator=g) * 0.1).to(cuda), golden.spk[b].to(cuda)) for b, m in enumerate(n)]
    out = {o[0]: o for o in model.generate_speech_stream(reqs, rows=2, max_src_len=32, need_attn=True, threshold=1.0)}
    assert len(out) == 3
    for key, src, spk in reqs:
        ref = model.generate_speech(source=src.unsqueeze(0), spkembs=spk.unsqueeze(0), threshold=1.0,
                                    padding_mask=torch.zeros(1, src.numel(), dtype=torch.bool, device=cuda))
        _same_as_single(out[key], ref, key)
    assert len({o[3].shape[-1] for o in out.values()}) == 3          # three different encoder lengths


# ---- text to waveform ----
def test_synthesize_stream_rows_equal_single_row_pipeline(cuda, golden, nine_singles):
    from speecht5_amd.task import SpeechT5Task
    from tests.test_tts_wave_gpu import _row_bar, _vocoder
    model, args = _tiny(cuda)
    vocoder, _, _ = _vocoder(cuda, "tiny", torch.float32)
    reqs = _nine(golden, args.reduction_factor, cuda)[:5]
    task = SpeechT5Task.synthetic(args)
    out = list(task.synthesize_stream([model], reqs, vocoder=vocoder, rows=2, max_src_len=32, threshold=2.0))
    assert sorted(o[0] for o in out) == sorted(q[0] for q in reqs)
    for key, wav, mel, probs in out:
        ref = nine_singles[int(key[1:])]
        _same_as_single((key, mel, probs, None), ref, key)
        assert wav.shape == (mel.shape[0] * vocoder._packed_rate(),)
        _row_bar(wav, vocoder(ref[0]), torch.float32, f"{key} wav")
    bare = list(model.synthesize_stream(reqs[:2], rows=2, max_src_len=32, threshold=2.0))
    assert all(o[1] is None for o in bare)
    got = list(task.generate_speech_stream([model], reqs[:2], rows=2, max_src_len=32, threshold=2.0))
    for o, b in zip(got, bare):
        assert o[0] == b[0] and o[3] is None
        close(o[1], b[2], 1e-5, what="mel without a vocoder")


# ---- refusals ----
def test_refusals(cuda, golden):
    model, args = _tiny(cuda)
    reqs = _nine(golden, args.reduction_factor, cuda)[1:4]
    with pytest.raises(ValueError, match="decode"):
        model.generate_speech_stream(reqs, rows=2, max_src_len=32, decode="eager")
    with pytest.raises(ValueError, match="rows"):
        model.generate_speech_stream(reqs, rows=0, max_src_len=32)
    with pytest.raises(ValueError, match="max_src_len"):
        model.generate_speech_stream(reqs, rows=2, max_src_len=0)
    model.train()
    with pytest.raises(ValueError, match="training mode"):
        model.generate_speech_stream(reqs, rows=2, max_src_len=32)
    model.eval()
    heads = model.decoder.layers[0].self_attn
    old = heads.head_dim
    heads.head_dim = 32                          # what tts_graph.unsupported_reason refuses
    try:
        with pytest.raises(ValueError, match="head_dim"):
            model.generate_speech_stream(reqs, rows=2, max_src_len=32)
    finally:
        heads.head_dim = old
    assert list(model.generate_speech_stream([], rows=2, max_src_len=32)) == []


def test_an_over_long_request_is_refused_by_key_while_the_others_complete(cuda, golden, nine_singles):
    model, args = _tiny(cuda)
    nine = _nine(golden, args.reduction_factor, cuda)
    S = 12 * args.reduction_factor // 2
    reqs = [nine[1], ("too long", nine[0][1], nine[0][2]), nine[4], nine[2]]
    got = []
    with pytest.raises(ValueError, match="'too long'.*max_src_len"):
        for o in model.generate_speech_stream(reqs, rows=2, max_src_len=S, threshold=2.0):
            got.append(o)
    assert sorted(o[0] for o in got) == ["u1", "u2", "u4"]
    for o in got:
        _same_as_single(o, nine_singles[int(o[0][1:])], o[0])


# ---- the batch path is not touched ----
def test_the_batch_path_gives_the_same_bits_before_and_after_a_stream(cuda, golden):
    model, args = _tiny(cuda)
    toks, spk = golden.toks.to(cuda), golden.spk.to(cuda)
    before = model.generate_speech_batch(src_tokens=toks, spkembs=spk, decode="graph", threshold=2.0)
    assert len(list(model.generate_speech_stream(_nine(golden, args.reduction_factor, cuda), rows=ROWS, max_src_len=32, threshold=2.0))) == 9
    after = model.generate_speech_batch(src_tokens=toks, spkembs=spk, decode="graph", threshold=2.0)
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
