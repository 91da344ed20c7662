"""Whole generate() calls with the beam step on the device: SequenceGenerator(decode="device") and decode="graph"
(speecht5_amd/beam_graph.py, csrc/beam_step.hip).

1. the cases beam1, beam3 and beam3_unnorm_minlen of tests/golden/tiny_s2t_beam.pt (hypotheses of the verbatim reference generator)
   under the comparison of tests/test_beam_slots_gpu.py::_assert_hyps, in both modes;
2. "graph" = "device" bit for bit (tokens, scores, positional scores) on a ragged batch of 3 sentences in which one finishes early;
   the graph is replayed, and the host polls exactly where tts_graph.replay_schedule says;
3. "device" against "slots" on that batch, fp32: identical best tokens, scores within the 2e-3 bar of profiles/beam_slots_parity.txt;
4. every option these modes refuse raises ValueError naming it; an unknown decode value still raises;
5. nothing moves: slot K/V, encoder-side K|V, ancestry table and hypothesis records have the same data pointers at the first and the
   last step.
Figures go to the file ST5_PARITY_OUT names."""
import os

import pytest
import torch

from tests.test_beam_slots_gpu import POS_TOL, _assert_hyps, _ragged_sample
from tests.util import Task, build_tiny, load_golden, to_dev

pytestmark = pytest.mark.gpu

RAGGED = dict(lengths=[7000, 2400, 6100], seed=21)
RAGGED_KW = dict(beam_size=3, max_len_b=30)
# The tiny model with the golden weights closes no hypothesis before the length limit and hardly looks at its input.  For the ragged
# batch its tied embedding's eos row is scaled (eos becomes likely after a few steps) and the cross-attention output projections are
# amplified (when it does depends on the sentence): the middle sentence then finishes at step 11, the others at step 17.
EOS_ROW_SCALE, CROSS_GAIN = -6.0, 8.0


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


def _report(line):
    print(line)
    path = os.environ.get("ST5_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def tiny(cuda):
    _, fx = load_golden("tiny_s2t_beam.pt")
    model, args = build_tiny(cuda, torch.float32)
    model.eval()
    return model, args, fx, Task().dicts["text"]


@pytest.fixture(scope="module")
def ragged(cuda, tiny):
    """The ragged batch decoded once per mode (shared by the tests below)."""
    from speecht5_amd import functional as Fn
    from speecht5_amd.sequence_generator import SequenceGenerator
    d = tiny[3]
    model, _ = build_tiny(cuda, torch.float32)
    model.eval()
    with torch.no_grad():
        model.text_decoder_prenet.embed_tokens.weight[d.eos()] *= EOS_ROW_SCALE
        for layer in model.decoder.layers:
            layer.encoder_attn.out_proj.weight *= CROSS_GAIN
    Fn.weight_cache.clear()
    sample = _ragged_sample(cuda, RAGGED["lengths"], RAGGED["seed"])
    out = {}
    for mode in ("slots", "device", "graph"):
        gen = SequenceGenerator([model], d, decode=mode, **RAGGED_KW)
        out[mode] = (gen, gen.generate([model], sample))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode", ["device", "graph"])
@pytest.mark.parametrize("name", ["beam1", "beam3", "beam3_unnorm_minlen"])
def test_golden_hypotheses(cuda, tiny, name, mode):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _, fx, d = tiny
    case = fx["cases"][name]
    assert case["prefix"] is None
    gen = SequenceGenerator([model], d, decode=mode, **case["kw"])
    hyps = gen.generate([model], to_dev(fx["samples"][case["sample"]], cuda))
    _assert_hyps(hyps, case["hyps"])
    assert gen.beam_decode_mode == mode
    for sent in hyps:
        for h in sent:
            assert h["tokens"].dtype == torch.int64 and h["attention"].numel() == 0 and h["alignment"].numel() == 0
            assert set(h) == {"tokens", "score", "attention", "alignment", "positional_scores"}


def _done_step(hyps, beam, max_len):
    """The step at which the last sentence finished: its `beam`-th hypothesis, or max_len."""
    return max(max(len(h["tokens"]) for h in sent) - 1 if len(sent) == beam else max_len for sent in hyps)


def test_graph_equals_device_bit_for_bit(ragged):
    from speecht5_amd.tts_graph import GRAPH_WARMUP_STEPS, replay_schedule
    (gd, dev), (gg, gra) = ragged["device"], ragged["graph"]
    assert len(dev) == len(gra) == 3
    for a, b in zip(dev, gra):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert torch.equal(x["tokens"], y["tokens"]) and torch.equal(x["score"], y["score"])
            assert torch.equal(x["positional_scores"], y["positional_scores"])
    beam, max_len = RAGGED_KW["beam_size"], RAGGED_KW["max_len_b"]
    ends = [max(len(h["tokens"]) for h in sent) - 1 for sent in dev]
    assert min(ends) < max(ends), f"one sentence must finish early (last steps {ends})"
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
    (_, slots), (_, dev) = ragged["slots"], ragged["device"]
    worst = worst_pos = 0.0
    for si, (a, b) in enumerate(zip(slots, dev)):
        assert a[0]["tokens"].tolist() == b[0]["tokens"].tolist(), f"sentence {si}: best hypothesis"
        worst = max(worst, abs(float(a[0]["score"]) - float(b[0]["score"])))
        worst_pos = max(worst_pos, float((a[0]["positional_scores"] - b[0]["positional_scores"]).abs().max()))
    _report(f"device vs slots (tiny, fp32, ragged 3 x beam 3): best score |d| {worst:.3e}  positional |d| {worst_pos:.3e}  bar {POS_TOL:.0e}")
    assert worst <= POS_TOL and worst_pos <= POS_TOL


def test_buffers_do_not_move(ragged):
    for mode in ("device", "graph"):
        first, last = ragged[mode][0].beam_buffer_ptrs
        assert first == last and len(first) >= 4 and all(first)


@pytest.mark.parametrize("mode", ["device", "graph"])
def test_refused_options_raise(cuda, tiny, mode):
    from speecht5_amd.sequence_generator import BeamSearch, SequenceGenerator
    model, _, fx, d = tiny
    other, _ = build_tiny(cuda, torch.float32)
    for kw, word in [(dict(ctc_weight=0.3), "ctc_weight"), (dict(lm_model=torch.nn.Identity()), "lm_model"),
                     (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(match_source_len=True), "match_source_len"),
                     (dict(search_strategy=BeamSearch(d)), "search_strategy"), (dict(beam_size=33), "beam_size")]:
        with pytest.raises(ValueError, match=word):
            SequenceGenerator([model], d, decode=mode, **({"beam_size": 2} | kw))
    with pytest.raises(ValueError, match="more than one model"):
        SequenceGenerator([model, other.eval()], d, decode=mode, beam_size=2)
    gen = SequenceGenerator([model], d, decode=mode, beam_size=2, max_len_b=6)
    sample = to_dev(fx["samples"]["two"], cuda)
    with pytest.raises(ValueError, match="prefix_tokens"):
        gen.generate([model], sample, prefix_tokens=torch.full((2, 1), 7, device=cuda))
    with pytest.raises(ValueError, match="constraints"):
        gen.generate([model], sample, constraints=torch.zeros(2, 1, device=cuda))
    sa = model.decoder.layers[0].self_attn
    hd = sa.head_dim
    try:
        sa.head_dim = 48                                  # a decoder that fails check_beam_slots
        with pytest.raises(ValueError, match="heads of 48"):
            SequenceGenerator([model], d, decode=mode, beam_size=2)
    finally:
        sa.head_dim = hd


def test_unknown_decode_still_raises(tiny):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, _, _, d = tiny
    with pytest.raises(ValueError, match="paged"):
        SequenceGenerator([model], d, decode="paged")
