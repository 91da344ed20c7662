"""SequenceGenerator.generate_stream (speecht5_amd/beam_stream.py) on the tiny model of tiny_s2t_beam.pt, with the EOS_ROW_SCALE /
CROSS_GAIN change of tests/test_beam_device_gpu.py so that sentences end by eos at data-dependent steps.  Nine requests of 2400 to 7000
samples with their own step limits go through 3 slots, at beam 2 and beam 5.

The reference arm of a request is generate(decode="graph", exact_rows=True) with max_len_b = the request's limit on a batch of that
one sentence, padded to max_src_len samples with its padding mask.

1. both modes: tokens, score and positional_scores of every hypothesis are bit-equal to the reference arm;
2. completion order, polls and tick count follow tts_stream.stream_schedule on the singles' step counts; the inputs are asserted to be
   non-trivial (three distinct finishing steps, an eos before the limit, a reused slot, two sentences at one poll);
3. a result does not depend on slot, admission tick or neighbours: two arrival orders, fp32 and bf16;
4. "graph" replays: beam_graph_replays > 0, the eager steps are GRAPH_WARMUP_STEPS, no baked-in buffer moves;
5. every refusal raises and names its option or key; an over-long request is refused by key while the others complete;
6. a generate(decode="graph") call gives the same bits before and after a stream."""
import pytest
import torch

from tests.test_beam_device_gpu import CROSS_GAIN, EOS_ROW_SCALE
from tests.util import Task, build_tiny

pytestmark = pytest.mark.gpu

LENGTHS = [7000, 2400, 6100, 3300, 5200, 2900, 6600, 4100, 4800]
LIMITS = [30, 9, 17, 5, 30, 12, 30, 7, 21]
MAX_SRC, SLOTS, CAP, SEED = 7000, 3, 30, 21
BEAMS = (2, 5)


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


def _model(cuda, dtype=torch.float32):
    from speecht5_amd import functional as Fn
    d = Task().dicts["text"]
    model, _ = build_tiny(cuda, dtype)
    model.eval()
    with torch.no_grad():
        model.text_decoder_prenet.embed_tokens.weight[d.eos()] *= EOS_ROW_SCALE
        for layer in model.decoder.layers:
            layer.encoder_attn.out_proj.weight *= CROSS_GAIN
    Fn.weight_cache.clear()
    return model, d


def _requests(cuda, order=None):
    g = torch.Generator().manual_seed(SEED)
    waves = [(torch.randn(n, generator=g) * 0.1).to(cuda) for n in LENGTHS]
    reqs = [(f"utt{i}", w, ml) for i, (w, ml) in enumerate(zip(waves, LIMITS))]
    return reqs if order is None else [reqs[i] for i in order]


def _single(model, d, cuda, beam, wav, limit, mode="graph"):
    from speecht5_amd.sequence_generator import SequenceGenerator
    src = torch.zeros(1, MAX_SRC, device=cuda)
    pad = torch.ones(1, MAX_SRC, dtype=torch.bool, device=cuda)
    src[0, :wav.numel()] = wav
    pad[0, :wav.numel()] = False
    gen = SequenceGenerator([model], d, decode=mode, exact_rows=True, beam_size=beam, max_len_b=limit)
    return gen.generate([model], {"net_input": {"source": src, "padding_mask": pad}})[0]


def _stream(model, d, beam, reqs, mode, **kw):
    from speecht5_amd.sequence_generator import SequenceGenerator
    gen = SequenceGenerator([model], d, beam_size=beam, max_len_b=CAP)
    out = list(gen.generate_stream(reqs, sentences=SLOTS, max_src_len=MAX_SRC, decode=mode, **kw))
    torch.cuda.synchronize()
    return gen, out


def _steps_of(hyps, beam, limit):
    return (max(len(h["tokens"]) for h in hyps) - 1 if len(hyps) == beam else limit) + 1


def _assert_same_hyps(got, want, what):
    assert len(got) == len(want) > 0, what
    for k, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b) == {"tokens", "score", "attention", "alignment", "positional_scores"}
        assert a["tokens"].dtype == torch.int64 and a["attention"].numel() == 0 and a["alignment"].numel() == 0
        assert torch.equal(a["tokens"], b["tokens"]), f"{what} hypothesis {k}: tokens"
        assert torch.equal(a["score"].view(torch.int32), b["score"].view(torch.int32)), f"{what} hypothesis {k}: score (bits)"
        assert torch.equal(a["positional_scores"].view(torch.int32), b["positional_scores"].view(torch.int32)), f"{what} hypothesis {k}: positional"


@pytest.fixture(scope="module")
def arms(cuda):
    """The model, the reference arm of every request and the stream in both modes, per beam (shared by the tests below)."""
    from speecht5_amd import functional as Fn
    model, d = _model(cuda)
    reqs = _requests(cuda)
    out = {"model": model, "d": d, "reqs": reqs}
    for beam in BEAMS:
        singles = {key: _single(model, d, cuda, beam, wav, ml) for key, wav, ml in reqs}
        streams = {mode: _stream(model, d, beam, reqs, mode) for mode in ("device", "graph")}
        out[beam] = (singles, streams)
    torch.cuda.synchronize()
    yield out
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


@pytest.mark.parametrize("mode", ["device", "graph"])
@pytest.mark.parametrize("beam", BEAMS)
def test_every_hypothesis_is_bit_equal_to_the_single_call(arms, beam, mode):
    singles, streams = arms[beam]
    _, out = streams[mode]
    assert sorted(k for k, _ in out) == sorted(singles)
    for key, hyps in out:
        _assert_same_hyps(hyps, singles[key], f"beam {beam} {mode} {key}")


@pytest.mark.parametrize("mode", ["device", "graph"])
@pytest.mark.parametrize("beam", BEAMS)
def test_completion_order_polls_and_ticks_follow_stream_schedule(arms, beam, mode):
    from speecht5_amd.tts_stream import stream_schedule
    singles, streams = arms[beam]
    gen, out = streams[mode]
    reqs = arms["reqs"]
    P = gen.BEAM_POLL_STEPS
    lengths = [_steps_of(singles[key], beam, ml) for key, _, ml in reqs]
    print(f"beam {beam} {mode}: steps {lengths} limits {LIMITS}")
    ticks, order, plan = stream_schedule(lengths, SLOTS, P, with_plan=True)
    assert [gen.beam_stream_stats["sentence_steps"][key] for key, _, _ in reqs] == lengths
    assert [k for k, _ in out] == [reqs[i][0] for i in order]
    assert gen.beam_device_steps + gen.beam_graph_replays == ticks and gen.beam_polls == ticks // P
    # the inputs are not trivial
    assert len(set(lengths)) >= 3, lengths
    assert any(n < ml + 1 for n, ml in zip(lengths, LIMITS)), "no sentence ended by eos before its limit"
    assert len(plan) > SLOTS and gen.beam_stream_stats["admitted"] == len(reqs)
    ends = [(t + lengths[i] + P - 1) // P for i, _, t in plan]
    assert len(set(ends)) < len(ends), "no poll at which two sentences finish"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_result_does_not_depend_on_slot_tick_or_neighbours(cuda, dtype):
    model, d = _model(cuda, dtype)
    beam = 5
    first = dict(_stream(model, d, beam, _requests(cuda), "graph")[1])
    second = dict(_stream(model, d, beam, _requests(cuda, order=[8, 3, 0, 6, 1, 7, 4, 2, 5]), "graph")[1])
    assert sorted(first) == sorted(second) and len(first) == len(LENGTHS)
    for key in first:
        _assert_same_hyps(second[key], first[key], f"{dtype} {key}")


@pytest.mark.parametrize("beam", BEAMS)
def test_graph_mode_replays_and_nothing_moves(arms, beam):
    from speecht5_amd.step_program import GRAPH_WARMUP_STEPS
    _, streams = arms[beam]
    gg, gd = streams["graph"][0], streams["device"][0]
    assert gg.beam_decode_mode == "graph" and gg.beam_graph_replays > 0 and gg.beam_device_steps == GRAPH_WARMUP_STEPS
    assert gd.beam_decode_mode == "device" and gd.beam_graph_replays == 0 and gd.beam_device_steps == gg.beam_device_steps + gg.beam_graph_replays
    for g in (gg, gd):
        first, last = g.beam_buffer_ptrs
        assert first == last and len(first) >= 8 and all(first)


def test_refusals_name_their_option(cuda, arms):
    from speecht5_amd.sequence_generator import BeamSearch, SequenceGenerator
    model, d, reqs = arms["model"], arms["d"], arms["reqs"]
    ok = dict(sentences=SLOTS, max_src_len=MAX_SRC)
    for kw, word in [(dict(ctc_weight=0.3), "ctc_weight"), (dict(ctc_weight=0.3, ctc_rows=True), "ctc_weight"),
                     (dict(lm_model=torch.nn.Identity()), "lm_model"), (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"),
                     (dict(match_source_len=True), "match_source_len"), (dict(search_strategy=BeamSearch(d)), "search_strategy"),
                     (dict(beam_size=33), "beam_size")]:
        gen = SequenceGenerator([model], d, **({"beam_size": 2} | kw))
        with pytest.raises(ValueError, match=word):
            gen.generate_stream(reqs, **ok)
    gen = SequenceGenerator([model], d, beam_size=5, max_len_b=CAP)
    for kw, word in [(dict(ok, decode="slots"), "decode"), (dict(ok, sentences=0), "sentences"), (dict(ok, sentences=7), "sentences"),
                     (dict(ok, max_src_len=0), "max_src_len"), (dict(ok, max_src_len=100), "max_src_len")]:
        with pytest.raises(ValueError, match=word):
            gen.generate_stream(reqs, **kw)


def test_refused_requests_are_named_while_the_others_complete(cuda, arms):
    model, d, reqs = arms["model"], arms["d"], arms["reqs"]
    singles, _ = arms[5]
    g = torch.Generator().manual_seed(3)
    mixed = [reqs[1], ("too long", (torch.randn(MAX_SRC + 1, generator=g) * 0.1).to(cuda)), reqs[3],
             ("integers", torch.zeros(3000, dtype=torch.int64, device=cuda)), ("limit", reqs[5][1], CAP + 1), reqs[7]]
    got = []
    with pytest.raises(ValueError) as err:
        from speecht5_amd.sequence_generator import SequenceGenerator
        from speecht5_amd.task import SpeechT5Task
        gen = SequenceGenerator([model], d, beam_size=5, max_len_b=CAP)
        # (the task's wrapper uses nothing of the task: called unbound, the test tasks of tests/util.py are no SpeechT5Task)
        for item in SpeechT5Task.inference_stream(None, gen, [model], mixed, sentences=2, max_src_len=MAX_SRC, decode="graph"):
            got.append(item)
    text = str(err.value)
    assert "'too long'" in text and "max_src_len" in text and "'integers'" in text and "'limit'" in text and "max_len" in text
    assert sorted(k for k, _ in got) == ["utt1", "utt3", "utt7"]
    for key, hyps in got:
        _assert_same_hyps(hyps, singles[key], key)


def test_generate_gives_the_same_bits_before_and_after_a_stream(cuda, arms):
    from tests.test_beam_device_gpu import RAGGED, RAGGED_KW
    from tests.test_beam_slots_gpu import _ragged_sample
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, d, reqs = arms["model"], arms["d"], arms["reqs"]
    sample = _ragged_sample(cuda, RAGGED["lengths"], RAGGED["seed"])
    gen = SequenceGenerator([model], d, decode="graph", **RAGGED_KW)
    before = gen.generate([model], sample)
    assert len(_stream(model, d, 5, reqs, "graph")[1]) == len(reqs)
    after = gen.generate([model], sample)
    assert len(before) == len(after) == 3
    for s, (a, b) in enumerate(zip(before, after)):
        _assert_same_hyps(b, a, f"sentence {s}")
