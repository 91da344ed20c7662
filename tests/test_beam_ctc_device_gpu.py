"""Whole generate() calls with joint CTC / attention scoring in the device-stepped modes: SequenceGenerator(decode="device" /
"graph", ctc_weight > 0, ctc_rows=True) (speecht5_amd/beam_graph.py, csrc/beam_ctc.hip).

1. the cases beam1_ctc05, beam3_ctc03 and beam4_ctc05 of tests/golden/tiny_s2t_beam.pt (hypotheses of the verbatim reference
   generator; one sentence, for which ctc_rows=True is the reference's scoring) under tests/test_beam_slots_gpu.py::_assert_hyps;
2. a ragged batch of 3 (tests/test_beam_device_gpu.py's clips made longer, see LENGTH_SCALE, with its weight edit) at beam 3,
   ctc_weight 0.4: "graph" = "device" bit for bit, the graph is replayed, the host polls where tts_graph.replay_schedule says; "device" against "slots" with the same options:
   identical best tokens, best and positional scores within POS_TOL.  The batch is first shown to be a fair one on the "slots" result
   alone: best and second-best scores more than 10 * POS_TOL apart, one sentence finishing before the others.  That run leaves the
   scores unnormalised; a second one with the default normalize_scores compares the sentences with a clear best hypothesis;
3. what stays refused, the buffers that must not move, and the library calls of a decode without CTC."""
import pytest
import torch

from tests.test_beam_device_gpu import CROSS_GAIN, EOS_ROW_SCALE, RAGGED, _done_step, _report
from tests.test_beam_slots_gpu import POS_TOL, _assert_hyps, _ragged_sample
from tests.test_ctc_rows_gpu import _count_lib_calls
from tests.util import Task, build_tiny, load_golden, to_dev

pytestmark = pytest.mark.gpu

# tests/test_beam_device_gpu.py's batch as it stands cannot be decoded with CTC on ANY path: its middle clip has 7 encoder frames and
# decodes past 7 labels, where every label extension has CTC probability zero, a hypothesis leaves its candidates and the generator
# raises its KeyError (decode="slots", seeds 1 .. 40: all of them).  The clips keep their proportions and are LENGTH_SCALE times as
# long.  The tiny model's three hypotheses of a sentence end within a few 1e-3 of each other per token, so the scores are left
# unnormalised (the sum over the tokens, a stricter object for the POS_TOL comparison as well) and the seed is one under which the
# "slots" result has the properties test_the_ragged_batch_is_a_fair_one asks for (scanned on MI355X).
LENGTH_SCALE, SEED = 2, 33
LENGTHS = [m * LENGTH_SCALE for m in RAGGED["lengths"]]
RAGGED_KW = dict(beam_size=3, max_len_b=30, ctc_weight=0.4, ctc_rows=True, normalize_scores=False)
CTC_STEP = ["st5_beam_ctc_candidates", "st5_ctc_prefix_score_rows_dev", "st5_beam_step_logprobs", "st5_ctc_select_dev"]


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


@pytest.fixture(scope="module")
def tiny(cuda):
    _, fx = load_golden("tiny_s2t_beam.pt")
    model, args = build_tiny(cuda, torch.float32)
    model.eval()
    return model, args, fx, Task().dicts["text"]


def _decode_ragged(cuda, d, kw):
    """The ragged batch decoded once per mode with the options `kw`."""
    from speecht5_amd import functional as Fn
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _ = build_tiny(cuda, torch.float32)
    model.eval()
    with torch.no_grad():
        model.text_decoder_prenet.embed_tokens.weight[d.eos()] *= EOS_ROW_SCALE
        for layer in model.decoder.layers:
            layer.encoder_attn.out_proj.weight *= CROSS_GAIN
    Fn.weight_cache.clear()
    sample = _ragged_sample(cuda, LENGTHS, SEED)
    out = {}
    for mode in ("slots", "device", "graph"):
        gen = SequenceGenerator([model], d, decode=mode, **kw)
        out[mode] = (gen, gen.generate([model], sample))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def ragged(cuda, tiny):
    """Unnormalised scores (shared by the tests below)."""
    return _decode_ragged(cuda, tiny[3], RAGGED_KW)


@pytest.fixture(scope="module")
def ragged_normalised(cuda, tiny):
    """The generator's default, scores divided by length ** len_penalty (the device step's len_div table)."""
    return _decode_ragged(cuda, tiny[3], {k: v for k, v in RAGGED_KW.items() if k != "normalize_scores"})


@pytest.mark.parametrize("mode", ["device", "graph"])
@pytest.mark.parametrize("name", ["beam1_ctc05", "beam3_ctc03", "beam4_ctc05"])
def test_golden_hypotheses(cuda, tiny, name, mode):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _, fx, d = tiny
    case = fx["cases"][name]
    assert case["prefix"] is None and case["kw"]["ctc_weight"] > 0 and case["sample"] == "one"
    gen = SequenceGenerator([model], d, decode=mode, ctc_rows=True, **case["kw"])
    hyps = gen.generate([model], to_dev(fx["samples"][case["sample"]], cuda))
    _assert_hyps(hyps, case["hyps"])
    assert gen.beam_decode_mode == mode


def test_the_ragged_batch_is_a_fair_one(ragged):
    """Properties of the input, read from the "slots" result alone."""
    _, slots = ragged["slots"]
    for si, sent in enumerate(slots):
        assert len(sent) >= 2 and float(sent[0]["score"]) - float(sent[1]["score"]) > 10 * POS_TOL, f"sentence {si}: best two too close"
    ends = [max(len(h["tokens"]) for h in sent) - 1 for sent in slots]
    assert min(ends) < max(ends), f"one sentence must finish early (last steps {ends})"


def test_graph_equals_device_bit_for_bit(ragged):
    from speecht5_amd.tts_graph import GRAPH_WARMUP_STEPS, replay_schedule
    test_the_ragged_batch_is_a_fair_one(ragged)
    (gd, dev), (gg, gra) = ragged["device"], ragged["graph"]
    assert len(dev) == len(gra) == 3
    for a, b in zip(dev, gra):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert torch.equal(x["tokens"], y["tokens"]) and torch.equal(x["score"], y["score"])
            assert torch.equal(x["positional_scores"], y["positional_scores"])
    beam, max_len = RAGGED_KW["beam_size"], RAGGED_KW["max_len_b"]
    assert gg.beam_graph_replays > 0 and gg.beam_device_steps == GRAPH_WARMUP_STEPS and gd.beam_graph_replays == 0
    done = _done_step(dev, beam, max_len)
    for gen, eager in ((gd, max_len + 1), (gg, GRAPH_WARMUP_STEPS)):
        polls = steps = 0
        for first, ne, nr, poll in replay_schedule(max_len + 1, gen.BEAM_POLL_STEPS, eager):
            steps = first + ne + nr - 1
            polls += poll
            if poll and steps >= done + 1:
                break
        assert gen.beam_polls == polls and gen.beam_device_steps + gen.beam_graph_replays == steps, (gen.beam_decode_mode, polls, steps)


def test_device_against_slots(ragged):
    test_the_ragged_batch_is_a_fair_one(ragged)
    (_, slots), (_, dev) = ragged["slots"], ragged["device"]
    worst = worst_pos = 0.0
    for si, (a, b) in enumerate(zip(slots, dev)):
        assert a[0]["tokens"].tolist() == b[0]["tokens"].tolist(), f"sentence {si}: best hypothesis"
        worst = max(worst, abs(float(a[0]["score"]) - float(b[0]["score"])))
        worst_pos = max(worst_pos, float((a[0]["positional_scores"] - b[0]["positional_scores"]).abs().max()))
    _report(f"device vs slots, ctc_weight 0.4 ctc_rows (tiny, fp32, ragged 3 x beam 3): best score |d| {worst:.3e}  positional |d| "
            f"{worst_pos:.3e}  bar {POS_TOL:.0e}")
    assert worst <= POS_TOL and worst_pos <= POS_TOL


def test_normalised_scores_on_the_ragged_batch(ragged_normalised):
    """The same batch with the default normalize_scores (len_div on the device, with CTC, on a batch).  "graph" = "device" bit for
    bit needs no margin.  Against "slots", a sentence is compared where the input is fair for it: its best and second-best "slots"
    scores more than 10 * POS_TOL apart (per token the tiny model's hypotheses are closer than that in most sentences; at least one
    sentence must qualify); there the best tokens are identical and the scores within POS_TOL.  Elsewhere the set of the `beam`
    hypotheses' scores must still agree within POS_TOL, whatever their order."""
    (_, slots), (_, dev), (_, gra) = (ragged_normalised[m] for m in ("slots", "device", "graph"))
    for a, b in zip(dev, gra):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert torch.equal(x["tokens"], y["tokens"]) and torch.equal(x["score"], y["score"])
            assert torch.equal(x["positional_scores"], y["positional_scores"])
    fair = 0
    for si, (a, b) in enumerate(zip(slots, dev)):
        assert len(a) == len(b)
        sa, sb = sorted(float(h["score"]) for h in a), sorted(float(h["score"]) for h in b)
        assert max(abs(x - y) for x, y in zip(sa, sb)) <= POS_TOL, f"sentence {si}: hypothesis scores"
        if len(a) >= 2 and float(a[0]["score"]) - float(a[1]["score"]) > 10 * POS_TOL:
            fair += 1
            assert a[0]["tokens"].tolist() == b[0]["tokens"].tolist(), f"sentence {si}: best hypothesis"
            assert abs(float(a[0]["score"]) - float(b[0]["score"])) <= POS_TOL
            assert float((a[0]["positional_scores"] - b[0]["positional_scores"]).abs().max()) <= POS_TOL
    assert fair >= 1, "no sentence with a clear best hypothesis: choose another seed"


def test_buffers_do_not_move_and_include_the_ctc_state(cuda, tiny, ragged):
    from speecht5_amd.sequence_generator import SequenceGenerator
    for mode in ("device", "graph"):
        first, last = ragged[mode][0].beam_buffer_ptrs
        assert first == last and all(first)
    model, _, fx, d = tiny                                   # (the same architecture without CTC: 9 pointers fewer)
    plain = SequenceGenerator([model], d, decode="device", beam_size=3, max_len_b=4)
    plain.generate([model], to_dev(fx["samples"]["one"], cuda))
    assert len(ragged["device"][0].beam_buffer_ptrs[0]) == len(plain.beam_buffer_ptrs[0]) + 9, "the 9 CTC buffers"


@pytest.mark.parametrize("mode", ["device", "graph"])
def test_what_stays_refused(cuda, tiny, mode):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _, _, d = tiny
    with pytest.raises(ValueError, match="ctc_weight"):
        SequenceGenerator([model], d, decode=mode, beam_size=2, ctc_weight=0.3)
    with pytest.raises(ValueError, match="ctc_rows=True"):
        SequenceGenerator([model], d, decode=mode, beam_size=2, ctc_weight=0.3, ctc_rows=False)
    with pytest.raises(ValueError, match="lm_model"):
        SequenceGenerator([model], d, decode=mode, beam_size=2, ctc_weight=0.3, ctc_rows=True, lm_model=torch.nn.Identity())
    SequenceGenerator([model], d, decode=mode, beam_size=2, ctc_weight=0.3, ctc_rows=True)


def _steps(log):
    """The library calls of a decode split at the pre-net launch that opens every step."""
    cut = [i for i, n in enumerate(log) if n == "st5_beam_embed_step"]
    return [log[a:b] for a, b in zip(cut, cut[1:] + [len(log)])]


def test_library_calls_without_ctc_are_unchanged(cuda, tiny):
    """ctc_weight = 0: every step is the same launch list, closed by the output projection, st5_beam_step and st5_beam_reorder_dev,
    with none of the CTC entries, whatever ctc_rows says.  With CTC the same list with the four CTC launches in the beam step's place."""
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _, fx, d = tiny
    sample = to_dev(fx["samples"]["one"], cuda)
    kw = dict(beam_size=3, max_len_b=9, decode="device")
    SequenceGenerator([model], d, **kw).generate([model], sample)                  # (first use fills the weight caches)
    h0, plain = _count_lib_calls(lambda: SequenceGenerator([model], d, **kw).generate([model], sample))
    h1, rows0 = _count_lib_calls(lambda: SequenceGenerator([model], d, ctc_rows=True, **kw).generate([model], sample))
    assert plain == rows0 and [h["tokens"].tolist() for h in h0[0]] == [h["tokens"].tolist() for h in h1[0]]
    assert not [n for n in plain if n.startswith("st5_ctc_") or n.startswith("st5_beam_ctc_") or n == "st5_beam_step_logprobs"]
    steps = _steps(plain)
    assert len(steps) > 1 and all(s == steps[0] for s in steps[:-1])
    assert steps[0][-3:] == ["st5_gemm_skinny", "st5_beam_step", "st5_beam_reorder_dev"] and steps[0].count("st5_beam_step") == 1
    SequenceGenerator([model], d, ctc_weight=0.3, ctc_rows=True, **kw).generate([model], sample)
    _, on = _count_lib_calls(lambda: SequenceGenerator([model], d, ctc_weight=0.3, ctc_rows=True, **kw).generate([model], sample))
    steps_on = _steps(on)
    assert len(steps_on) > 1 and all(s == steps_on[0] for s in steps_on[:-1])
    assert steps_on[0] == steps[0][:-2] + CTC_STEP + ["st5_beam_reorder_dev"]
