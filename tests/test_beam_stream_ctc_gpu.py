"""SequenceGenerator.generate_stream(joint_ctc=True) (speecht5_amd/beam_stream.py, the per-slot CTC kernels of csrc/beam_ctc.hip) on the
tiny model with the weight edit of tests/test_beam_device_gpu.py: whole streams of 3 slots at beams 2 and 5, ctc_weight 0.4.

The reference arm of a request is generate(decode="graph", exact_rows=True, ctc_rows=True, ctc_weight=0.4) with max_len_b = the
request's limit on a batch of that one sentence, padded to max_src_len samples with its padding mask.

tests/test_beam_ctc_device_gpu.py explains why short clips with long limits cannot be decoded with CTC at all: past as many labels as
the clip has encoder frames every extension has CTC probability zero and a hypothesis leaves its candidates.  So the limits here stay
at or below the clips' frame counts (21, 11, 18, 10, 16, 8, 20, 12, 14), except for ONE designated request (SHORT: 3 frames, limit
21).  At beam 2 (ctc_beam = 14 of the 36 symbols) its single call raises the generator's KeyError.  At beam 5 ctc_beam = min(36, 7 * 5) =
35: the candidates of a row are the whole dictionary but its lowest never-symbol, so NO single call on this model can leave them;
there SHORT decodes, its non-eos extensions impossible past 3 labels, and is the sentence that ends by eos long before its limit.  With
CTC in the score an eos far from the last frame is costly, so the other sentences mostly run to their limits; those whose limit is
near their frame count end by eos a step or two early.  Lengths, limits and seed were chosen on MI355X so that the reference arm
alone has the properties test_the_reference_arm_is_a_fair_input asserts.

1. both modes: tokens, score and positional_scores of every hypothesis are bit-equal to the reference arm;
2. two arrival orders, fp32 and bf16, give the same bits per key;
3. the graph is replayed and no baked-in buffer moves, the CTC ones included;
4. the designated request is named in the stream's KeyError while all others complete bit-equal;
5. the refusals name their option: joint_ctc without ctc_weight, without ctc_rows, lm_model under joint_ctc, an oversized state;
6. a stream without the keyword makes the library calls of the attention-only step; with it the four CTC launches take the beam
   step's place;
7. generate(decode="graph", ctc...) gives the same bits before and after a stream."""
import pytest
import torch

from tests.test_beam_stream_gpu import _assert_same_hyps, _model, _steps_of
from tests.test_ctc_rows_gpu import _count_lib_calls

pytestmark = pytest.mark.gpu

LENGTHS = [7000, 3600, 6100, 3300, 5200, 2900, 6600, 4100, 4800]
LIMITS = [21, 11, 14, 5, 16, 8, 12, 12, 9]
SHORT = ("short", 1300, 21)                  # the designated request: (key, samples, limit)
MAX_SRC, SLOTS, CAP, SEED, CTC_WEIGHT = 7000, 3, 21, 1, 0.4
BEAMS = (2, 5)
FAILS = {2: [SHORT[0]], 5: []}            # the requests whose single call raises KeyError, per beam (module docstring)
CTC_KW = dict(ctc_weight=CTC_WEIGHT, ctc_rows=True)
CTC_STEP_SENTS = ["st5_beam_ctc_candidates_sents", "st5_ctc_prefix_score_rows_sents", "st5_beam_step_sents_logprobs",
                  "st5_ctc_select_sents"]


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


def _requests(cuda, order=None, short=True, seed=None):
    g = torch.Generator().manual_seed(SEED if seed is None else seed)
    waves = [(torch.randn(n, generator=g) * 0.1).to(cuda) for n in LENGTHS + [SHORT[1]]]
    reqs = [(f"utt{i}", w, ml) for i, (w, ml) in enumerate(zip(waves, LIMITS))]
    reqs = reqs if order is None else [reqs[i] for i in order]
    return reqs + [(SHORT[0], waves[-1], SHORT[2])] if short else reqs       # (the designated request arrives last)


def _single(model, d, cuda, beam, wav, limit, **kw):
    """The reference arm: KeyError -> the exception, else the sentence's hypotheses."""
    from speecht5_amd.sequence_generator import SequenceGenerator
    src = torch.zeros(1, MAX_SRC, device=cuda)
    pad = torch.ones(1, MAX_SRC, dtype=torch.bool, device=cuda)
    src[0, :wav.numel()] = wav
    pad[0, :wav.numel()] = False
    gen = SequenceGenerator([model], d, decode="graph", exact_rows=True, beam_size=beam, max_len_b=limit, **kw)
    try:
        return gen.generate([model], {"net_input": {"source": src, "padding_mask": pad}})[0]
    except KeyError as e:
        torch.cuda.synchronize()
        return e


def _stream(model, d, beam, reqs, mode, **kw):
    """(generator, results, the stream's KeyError or None)."""
    from speecht5_amd.sequence_generator import SequenceGenerator
    gen = SequenceGenerator([model], d, beam_size=beam, max_len_b=CAP, **CTC_KW)
    out, err = [], None
    try:
        for item in gen.generate_stream(reqs, sentences=SLOTS, max_src_len=MAX_SRC, decode=mode, joint_ctc=True, **kw):
            out.append(item)
    except KeyError as e:
        err = e
    torch.cuda.synchronize()
    return gen, out, err


@pytest.fixture(scope="module")
def arms(cuda):
    """The model, the reference arm of every request (with CTC and, for the best hypothesis, without) and the stream in both modes,
    per beam (computed once, shared by the tests below, never changed)."""
    from speecht5_amd import functional as Fn
    model, d = _model(cuda)
    reqs = _requests(cuda)
    out = {"model": model, "d": d, "reqs": reqs}
    for beam in BEAMS:
        singles = {key: _single(model, d, cuda, beam, wav, ml, **CTC_KW) for key, wav, ml in reqs}
        plain = {key: _single(model, d, cuda, beam, wav, ml) for key, wav, ml in reqs}
        streams = {mode: _stream(model, d, beam, reqs, mode) for mode in ("device", "graph")}
        out[beam] = (singles, plain, streams)
    torch.cuda.synchronize()
    yield out
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


@pytest.mark.parametrize("beam", BEAMS)
def test_the_reference_arm_is_a_fair_input(arms, beam):
    """Read from the reference arm alone."""
    from speecht5_amd.sequence_generator import SequenceGenerator
    from speecht5_amd.tts_stream import stream_schedule
    singles, plain, _ = arms[beam]
    reqs = arms["reqs"]
    bad = [key for key, h in singles.items() if isinstance(h, KeyError)]
    assert bad == FAILS[beam], f"requests whose single call raises KeyError: {bad}"
    assert all("ctc_beam" in str(singles[key]) for key in bad)
    ok = [(key, ml) for key, _, ml in reqs if key not in bad]
    lengths = [_steps_of(singles[key], beam, ml) for key, ml in ok]
    print(f"beam {beam}: steps {lengths} limits {[ml for _, ml in ok]}")
    assert len(set(lengths)) >= 3, lengths
    assert any(n < ml + 1 for n, (_, ml) in zip(lengths, ok)), "no sentence ended by eos before its limit"
    P = SequenceGenerator.BEAM_POLL_STEPS
    _, _, plan = stream_schedule(lengths, SLOTS, P, with_plan=True)
    assert len(plan) > SLOTS, "no slot is reused"
    ends = [(t + lengths[i] + P - 1) // P for i, _, t in plan]
    assert len(set(ends)) < len(ends), "no poll at which two sentences finish"
    differs = [key for key, _ in ok if singles[key][0]["tokens"].tolist() != plain[key][0]["tokens"].tolist()]
    print(f"beam {beam}: best hypothesis differs from ctc_weight = 0 for {differs}")
    assert differs, "CTC changes no best hypothesis: a stream that ignored it would pass"


@pytest.mark.parametrize("mode", ["device", "graph"])
@pytest.mark.parametrize("beam", BEAMS)
def test_every_hypothesis_is_bit_equal_and_the_short_request_fails_by_key(arms, beam, mode):
    singles, _, streams = arms[beam]
    gen, out, err = streams[mode]
    bad = [key for key, h in singles.items() if isinstance(h, KeyError)]
    assert sorted(k for k, _ in out) == sorted(k for k in singles if k not in bad)
    for key, hyps in out:
        _assert_same_hyps(hyps, singles[key], f"beam {beam} {mode} {key}")
    assert gen.beam_stream_stats["failed"] == bad and gen.beam_stream_stats["admitted"] == len(singles)
    if bad:
        assert isinstance(err, KeyError) and all(repr(key) in str(err) for key in bad) and "ctc_beam" in str(err)
    else:
        assert err is None


@pytest.mark.parametrize("beam,dtype", [(5, torch.float32), (5, torch.bfloat16), (2, torch.float32)], ids=["b5-fp32", "b5-bf16", "b2-fp32"])
def test_a_result_does_not_depend_on_slot_tick_or_neighbours(cuda, beam, dtype):
    model, d = _model(cuda, dtype)
    _, first, e1 = _stream(model, d, beam, _requests(cuda), "graph")
    _, second, e2 = _stream(model, d, beam, _requests(cuda, order=[8, 3, 0, 6, 1, 7, 4, 2, 5]), "graph")
    first, second = dict(first), dict(second)
    assert sorted(first) == sorted(second) and len(first) == len(LENGTHS) + 1 - len(FAILS[beam])
    for key in first:
        _assert_same_hyps(second[key], first[key], f"{dtype} {key}")
    for e in (e1, e2):
        assert (isinstance(e, KeyError) and repr(SHORT[0]) in str(e)) if FAILS[beam] else e is None


@pytest.mark.parametrize("beam", BEAMS)
def test_graph_mode_replays_and_nothing_moves(cuda, arms, beam):
    from speecht5_amd.sequence_generator import SequenceGenerator
    from speecht5_amd.step_program import GRAPH_WARMUP_STEPS
    _, _, streams = arms[beam]
    gg, gd = streams["graph"][0], streams["device"][0]
    assert gg.beam_decode_mode == "graph" and gg.beam_graph_replays > 0 and gg.beam_device_steps == GRAPH_WARMUP_STEPS
    assert gd.beam_decode_mode == "device" and gd.beam_graph_replays == 0 and gd.beam_device_steps == gg.beam_device_steps + gg.beam_graph_replays
    for g in (gg, gd):
        first, last = g.beam_buffer_ptrs
        assert first == last and all(first)
    if beam == BEAMS[0]:                                      # (the same stream without CTC: 9 pointers fewer)
        model, d, reqs = arms["model"], arms["d"], arms["reqs"]
        plain = SequenceGenerator([model], d, beam_size=beam, max_len_b=CAP)
        assert len(list(plain.generate_stream(reqs[:2], sentences=SLOTS, max_src_len=MAX_SRC, decode="device"))) == 2
        assert len(gd.beam_buffer_ptrs[0]) == len(plain.beam_buffer_ptrs[0]) + 9, "the 9 CTC buffers"


def test_refusals_name_their_option(cuda, arms, monkeypatch):
    from speecht5_amd import functional as Fn
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, d, reqs = arms["model"], arms["d"], arms["reqs"]
    ok = dict(sentences=SLOTS, max_src_len=MAX_SRC, joint_ctc=True)
    for kw, word in [(dict(), "joint_ctc"), (dict(ctc_weight=0.3), "ctc_rows"),
                     (dict(ctc_weight=0.3, ctc_rows=True, lm_model=torch.nn.Identity()), "lm_model")]:
        gen = SequenceGenerator([model], d, **({"beam_size": 2} | kw))
        with pytest.raises(ValueError, match=word):
            gen.generate_stream(reqs, **ok)
    # without the keyword the refusal stands and points at it
    gen = SequenceGenerator([model], d, beam_size=2, **CTC_KW)
    with pytest.raises(ValueError, match="ctc_weight.*joint_ctc"):
        gen.generate_stream(reqs, sentences=SLOTS, max_src_len=MAX_SRC)
    # an oversized state names what sizes it
    monkeypatch.setattr(Fn, "BEAM_CTC_MAX_STATE_BYTES", 1 << 12)
    gen = SequenceGenerator([model], d, beam_size=2, max_len_b=CAP, **CTC_KW)
    with pytest.raises(ValueError, match="sentences.*max_src_len"):
        list(gen.generate_stream(reqs[:1], **ok))
    torch.cuda.synchronize()


def _steps(log):
    cut = [i for i, n in enumerate(log) if n == "st5_beam_embed_sents"]
    return [log[a:b] for a, b in zip(cut, cut[1:] + [len(log)])], log[:cut[0]]


def test_library_calls_without_the_keyword_are_the_attention_only_step(cuda, arms):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, d = arms["model"], arms["d"]
    reqs = _requests(cuda, short=False)[:2]

    def run(joint):
        gen = SequenceGenerator([model], d, beam_size=2, max_len_b=CAP, **(CTC_KW if joint else {}))
        return list(gen.generate_stream(reqs, sentences=2, max_src_len=MAX_SRC, decode="device", **(dict(joint_ctc=True) if joint else {})))

    _, off = _count_lib_calls(lambda: run(False))
    _, on = _count_lib_calls(lambda: run(True))
    steps, head = _steps(off)
    assert not [n for n in off if n.startswith("st5_ctc_") or n.startswith("st5_beam_ctc_") or n == "st5_beam_step_sents_logprobs"]
    assert head.count("st5_beam_sents_admit") == 1 and len(steps) > 1
    assert steps[0][-3:] == ["st5_gemm_skinny", "st5_beam_step_sents", "st5_beam_reorder_sents"]
    assert all(s[:len(steps[0])] == steps[0] for s in steps)
    steps_on, head_on = _steps(on)
    assert steps_on[0] == steps[0][:-2] + CTC_STEP_SENTS + ["st5_beam_reorder_sents"]
    assert all(s[:len(steps_on[0])] == steps_on[0] for s in steps_on)
    k = head_on.index("st5_beam_sents_admit")
    assert head_on[k + 1] == "st5_ctc_sents_admit" and head_on.count("st5_ctc_sents_admit") == 1


def test_generate_gives_the_same_bits_before_and_after_a_stream(cuda, arms):
    from tests.test_beam_ctc_device_gpu import LENGTHS as RAGGED_LENGTHS, RAGGED_KW, SEED as RAGGED_SEED
    from tests.test_beam_slots_gpu import _ragged_sample
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, d = arms["model"], arms["d"]
    sample = _ragged_sample(cuda, RAGGED_LENGTHS, RAGGED_SEED)
    gen = SequenceGenerator([model], d, decode="graph", **RAGGED_KW)
    before = gen.generate([model], sample)
    assert len(_stream(model, d, 5, _requests(cuda, short=False), "graph")[1]) == len(LENGTHS)
    after = gen.generate([model], sample)
    assert len(before) == len(after) == 3
    for s, (a, b) in enumerate(zip(before, after)):
        _assert_same_hyps(b, a, f"sentence {s}")
