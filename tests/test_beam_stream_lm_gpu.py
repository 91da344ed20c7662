"""SequenceGenerator.generate_stream with an lm_model (speecht5_amd/beam_stream.py, TransformerLanguageModel.device_step_sents,
st5_beam_lm_logprobs_sents of csrc/beam_lm.hip) on the tiny model with the weight edit of tests/test_beam_stream_gpu.py: whole streams
of 3 slots at beams 2 and 5 in fp32, attention + LM ("att") and attention + CTC + LM ("ctc").

The reference arm of a request is generate(decode="graph", exact_rows=True, lm_model=lm, lm_weight=LM_WEIGHT, max_len_b=limit) on a
batch of that one sentence, padded to max_src_len samples with its padding mask; with ctc_rows=True, ctc_weight=0.4 for "ctc".
"att" decodes the requests of tests/test_beam_stream_gpu.py (its LENGTHS, LIMITS, slot count and weight edit), "ctc" those of
tests/test_beam_stream_ctc_gpu.py without its SHORT request (limits at or below the clips' frame counts, for the reason that file's
docstring gives).  The LM is the fixture LM of tests/golden/tiny_s2t_beam_lm.pt (34 symbols under the model's 36: V_lm < V); one run
uses tests/test_beam_lm_device_gpu.py's LM with a tied output projection.

LM_WEIGHT and the seed of the "ctc" requests were chosen on MI355X so that the reference arm alone has the properties
test_the_reference_arm_is_a_fair_input asserts.  The fixture LM needs no scaling of its output projection: at its own weights it
changes the best hypothesis of all nine requests, under both scorings and beams.  At the recipe's lm_weight 0.5 the LM's dislike of
eos keeps every "att" sentence running to its limit (no eos before a limit), so LM_WEIGHT is 0.3, the weight of
tests/test_beam_lm_device_gpu.py.  With CTC and the LM at beam 2 (ctc_beam = 14 of 36 symbols) the requests of
tests/test_beam_stream_ctc_gpu.py's own seed include one whose single call raises the generator's KeyError (a hypothesis leaves its
CTC candidates); of the seeds 1 .. 40 scanned with the same LENGTHS and LIMITS, 6, 23 and 32 decode all nine requests at both beams
and meet every property, and CTC_SEED is the first of them.

1. the reference arm is a fair input (read from it alone, the values printed);
2. both modes, both scorings: tokens, score and positional_scores of every hypothesis are bit-equal to the reference arm;
3. two arrival orders, fp32 and bf16 at both beams, give the same bits per key: a result depends on neither slot, admission tick nor
   neighbours, which also pins that a handed-over slot's stale LM caches are never read (device_step_sents' docstring); the
   sentences that leave their CTC candidates in bf16 at beam 2 fail by key in both orders alike;
4. graph mode replays and no baked-in buffer moves, the LM's included;
5. the library calls: without an LM what the stream makes now; with one, one st5_beam_lm_logprobs_sents per step in beam_graph.py's
   order;
6. generate(decode="graph", lm_model=...) gives the same bits before and after a stream;
7. an LM with a tied output projection."""
import pytest
import torch

from tests import test_beam_stream_ctc_gpu as C
from tests import test_beam_stream_gpu as A
from tests.test_beam_lm_device_gpu import _tied_lm, _tiny_lm
from tests.test_beam_stream_gpu import _assert_same_hyps, _model, _steps_of
from tests.test_ctc_rows_gpu import _count_lib_calls
from tests.util import load_golden

pytestmark = pytest.mark.gpu

LM_WEIGHT, CTC_SEED, TIED_SEED = 0.3, 6, 1
MAX_SRC, SLOTS = A.MAX_SRC, A.SLOTS
BEAMS = (2, 5)
SCORINGS = ("att", "ctc")
CAPS = {"att": A.CAP, "ctc": C.CAP}
CTC_KW = {"att": {}, "ctc": C.CTC_KW}
ORDER = [8, 3, 0, 6, 1, 7, 4, 2, 5]
LM_LAYER_ROWS = ["st5_layernorm_fwd", "st5_gemm_skinny", "st5_gemm_skinny_rows", "st5_lm_decode_attn_rows", "st5_gemm_skinny",
                 "st5_layernorm_fwd", "st5_gemm_skinny", "st5_gemm_skinny"]
assert MAX_SRC == C.MAX_SRC and SLOTS == C.SLOTS


@pytest.fixture(autouse=True)
def _restore_fp32():
    yield
    from speecht5_amd import functional as Fn
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


def _lm(cuda):
    _, fx_lm = load_golden("tiny_s2t_beam_lm.pt")
    return _tiny_lm(fx_lm, cuda)


def _requests(cuda, scoring, order=None):
    return A._requests(cuda, order) if scoring == "att" else C._requests(cuda, order, short=False, seed=CTC_SEED)


def _single(model, d, cuda, beam, wav, limit, **kw):
    """The reference arm of one request."""
    from speecht5_amd.sequence_generator import SequenceGenerator
    src = torch.zeros(1, MAX_SRC, device=cuda)
    pad = torch.ones(1, MAX_SRC, dtype=torch.bool, device=cuda)
    src[0, :wav.numel()] = wav
    pad[0, :wav.numel()] = False
    gen = SequenceGenerator([model], d, decode="graph", exact_rows=True, beam_size=beam, max_len_b=limit, **kw)
    return gen.generate([model], {"net_input": {"source": src, "padding_mask": pad}})[0]


def _stream(model, d, lm, scoring, beam, reqs, mode, weight=LM_WEIGHT):
    from speecht5_amd.sequence_generator import SequenceGenerator
    gen = SequenceGenerator([model], d, beam_size=beam, max_len_b=CAPS[scoring], lm_model=lm, lm_weight=weight, **CTC_KW[scoring])
    out = list(gen.generate_stream(reqs, sentences=SLOTS, max_src_len=MAX_SRC, decode=mode, **(dict(joint_ctc=True) if scoring == "ctc" else {})))
    torch.cuda.synchronize()
    return gen, out


def _fair(singles, plain, reqs, beam):
    """What test_the_reference_arm_is_a_fair_input reads from the reference arm: (step counts, eos before the limit, a reused slot, two
    sentences at one poll, the keys whose best hypothesis the LM changes)."""
    from speecht5_amd.sequence_generator import SequenceGenerator
    from speecht5_amd.tts_stream import stream_schedule
    lengths = [_steps_of(singles[key], beam, ml) for key, _, ml in reqs]
    early = any(n < ml + 1 for n, (_, _, ml) in zip(lengths, reqs))
    P = SequenceGenerator.BEAM_POLL_STEPS
    _, _, plan = stream_schedule(lengths, SLOTS, P, with_plan=True)
    ends = [(t + lengths[i] + P - 1) // P for i, _, t in plan]
    differs = [key for key, _, _ in reqs if singles[key][0]["tokens"].tolist() != plain[key][0]["tokens"].tolist()]
    return lengths, early, len(plan) > SLOTS, len(set(ends)) < len(ends), differs


@pytest.fixture(scope="module")
def arms(cuda):
    """The model, the LM, the reference arm of every request (with the LM and, for the best hypothesis, without) and the stream in
    both modes, per scoring and beam (computed once, shared by the tests below, never changed)."""
    from speecht5_amd import functional as Fn
    model, d = _model(cuda)
    lm = _lm(cuda)

    class Arms(dict):
        def __missing__(self, key):                  # (scoring, beam): on first use
            scoring, beam = key
            reqs = self[scoring]
            kw = dict(lm_model=lm, lm_weight=LM_WEIGHT, **CTC_KW[scoring])
            singles = {k: _single(model, d, cuda, beam, wav, ml, **kw) for k, wav, ml in reqs}
            plain = {k: _single(model, d, cuda, beam, wav, ml, **CTC_KW[scoring]) for k, wav, ml in reqs}
            streams = {mode: _stream(model, d, lm, scoring, beam, reqs, mode) for mode in ("device", "graph")}
            torch.cuda.synchronize()
            self[key] = (singles, plain, streams)
            return self[key]

    out = Arms(model=model, d=d, lm=lm, **{scoring: _requests(cuda, scoring) for scoring in SCORINGS})
    yield out
    Fn.set_compute_dtype(torch.float32)
    Fn.weight_cache.clear()


@pytest.mark.parametrize("beam", BEAMS)
@pytest.mark.parametrize("scoring", SCORINGS)
def test_the_reference_arm_is_a_fair_input(arms, scoring, beam):
    """Read from the reference arm alone."""
    singles, plain, _ = arms[scoring, beam]
    reqs = arms[scoring]
    lengths, early, reused, together, differs = _fair(singles, plain, reqs, beam)
    print(f"{scoring} beam {beam}: steps {lengths} limits {[ml for _, _, ml in reqs]}; best hypothesis differs from lm_model=None for {differs}")
    assert len(set(lengths)) >= 3, lengths
    assert early, "no sentence ended by eos before its limit"
    assert reused, "no slot is reused"
    assert together, "no poll at which two sentences finish"
    assert differs, "the LM changes no best hypothesis: a stream that ignored it would pass"


@pytest.mark.parametrize("mode", ["device", "graph"])
@pytest.mark.parametrize("beam", BEAMS)
@pytest.mark.parametrize("scoring", SCORINGS)
def test_every_hypothesis_is_bit_equal_to_the_single_call(arms, scoring, beam, mode):
    singles, _, streams = arms[scoring, beam]
    gen, out = streams[mode]
    assert sorted(k for k, _ in out) == sorted(singles)
    for key, hyps in out:
        _assert_same_hyps(hyps, singles[key], f"{scoring} beam {beam} {mode} {key}")
    assert gen.beam_stream_stats["admitted"] == len(singles) and not gen.beam_stream_stats.get("failed")


@pytest.mark.parametrize("scoring,beam,dtype", [("att", 5, torch.float32), ("att", 5, torch.bfloat16), ("ctc", 5, torch.float32),
                                                ("ctc", 5, torch.bfloat16), ("att", 2, torch.float32), ("att", 2, torch.bfloat16),
                                                ("ctc", 2, torch.float32), ("ctc", 2, torch.bfloat16)],
                         ids=["att-b5-fp32", "att-b5-bf16", "ctc-b5-fp32", "ctc-b5-bf16", "att-b2-fp32", "att-b2-bf16", "ctc-b2-fp32",
                              "ctc-b2-bf16"])
def test_a_result_does_not_depend_on_slot_tick_or_neighbours(cuda, scoring, beam, dtype):
    """CTC_SEED was chosen in fp32.  With CTC at beam 2 (ctc_beam = 14 of 36 symbols) bf16 arithmetic lets a hypothesis of some
    requests leave its CTC candidates (utt1 and utt7 on MI355X): those sentences fail by key (tests/test_beam_stream_ctc_gpu.py), in
    both arrival orders alike, and the others are compared.  Every other case completes all nine requests."""
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, d = _model(cuda, dtype)
    lm = _lm(cuda)

    def run(order):
        gen = SequenceGenerator([model], d, beam_size=beam, max_len_b=CAPS[scoring], lm_model=lm, lm_weight=LM_WEIGHT, **CTC_KW[scoring])
        out = {}
        try:
            for key, hyps in gen.generate_stream(_requests(cuda, scoring, order), sentences=SLOTS, max_src_len=MAX_SRC, decode="graph",
                                                 **(dict(joint_ctc=True) if scoring == "ctc" else {})):
                out[key] = hyps
        except KeyError as e:
            assert "ctc_beam" in str(e)
        torch.cuda.synchronize()
        return out, sorted(gen.beam_stream_stats.get("failed", []))

    (first, failed), (second, failed2) = run(None), run(ORDER)
    print(f"{scoring} beam {beam} {dtype}: sentences that left their CTC candidates: {failed}")
    assert failed == failed2 and sorted(first) == sorted(second) and len(first) == len(ORDER) - len(failed) > 0
    if not (scoring == "ctc" and beam == 2 and dtype == torch.bfloat16):
        assert not failed
    for key in first:
        _assert_same_hyps(second[key], first[key], f"{scoring} {dtype} {key}")


@pytest.mark.parametrize("beam", BEAMS)
@pytest.mark.parametrize("scoring", SCORINGS)
def test_graph_mode_replays_and_nothing_moves(arms, scoring, beam):
    from speecht5_amd.sequence_generator import SequenceGenerator
    from speecht5_amd.step_program import GRAPH_WARMUP_STEPS
    _, _, streams = arms[scoring, beam]
    gg, gd = streams["graph"][0], streams["device"][0]
    assert gg.beam_decode_mode == "graph" and gg.beam_graph_replays > 0 and gg.beam_device_steps == GRAPH_WARMUP_STEPS
    assert gd.beam_decode_mode == "device" and gd.beam_graph_replays == 0 and gd.beam_device_steps == gg.beam_device_steps + gg.beam_graph_replays
    for g in (gg, gd):
        first, last = g.beam_buffer_ptrs
        assert first == last and all(first)
    if beam == BEAMS[0]:
        # the same stream without an LM: the LM's slot caches (one per layer) and its logits fewer; without CTC also the fused lp
        model, d, lm, reqs = arms["model"], arms["d"], arms["lm"], arms[scoring]
        no_lm = SequenceGenerator([model], d, beam_size=beam, max_len_b=CAPS[scoring], **CTC_KW[scoring])
        kw = dict(joint_ctc=True) if scoring == "ctc" else {}
        assert len(list(no_lm.generate_stream(reqs[:2], sentences=SLOTS, max_src_len=MAX_SRC, decode="device", **kw))) == 2
        more = len(lm.decoder.layers) + 1 + (0 if scoring == "ctc" else 1)
        assert len(gd.beam_buffer_ptrs[0]) == len(no_lm.beam_buffer_ptrs[0]) + more


def _steps(log, per):
    """The library calls of a stream split at the decoder's pre-net launch: every `per`-th st5_beam_embed_sents opens a step."""
    cut = [i for i, n in enumerate(log) if n == "st5_beam_embed_sents"]
    head, cut = log[:cut[0]], cut[::per]
    return [log[a:b] for a, b in zip(cut, cut[1:] + [len(log)])], head


def test_library_calls_of_a_step(cuda, arms):
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, d, lm = arms["model"], arms["d"], arms["lm"]
    lists, heads = {}, {}
    for name, scoring, with_lm in (("plain", "att", False), ("ctc", "ctc", False), ("lm", "att", True), ("lm_ctc", "ctc", True)):
        reqs = _requests(cuda, scoring)[:2]
        kw = dict(CTC_KW[scoring], **(dict(lm_model=lm, lm_weight=LM_WEIGHT) if with_lm else {}))
        skw = dict(joint_ctc=True) if scoring == "ctc" else {}

        def run():
            gen = SequenceGenerator([model], d, beam_size=2, max_len_b=CAPS[scoring], **kw)
            return list(gen.generate_stream(reqs, sentences=2, max_src_len=MAX_SRC, decode="device", **skw))

        run()                                                                # (first use fills the weight caches)
        _, log = _count_lib_calls(run)
        steps, heads[name] = _steps(log, 2 if with_lm else 1)
        n = len(steps[0])
        assert len(steps) > 1 and all(s[:n] == steps[0] for s in steps), f"{name}: every step is the same list"
        assert all(s.count("st5_beam_lm_logprobs_sents") == int(with_lm) for s in steps), f"{name}: one LM term per step"
        lists[name] = steps[0]
    plain, ctc = lists["plain"], lists["ctc"]
    # without an LM: what tests/test_beam_stream_ctc_gpu.py pins
    assert plain[-3:] == ["st5_gemm_skinny", "st5_beam_step_sents", "st5_beam_reorder_sents"] and plain.count("st5_beam_embed_sents") == 1
    assert ctc == plain[:-2] + C.CTC_STEP_SENTS + ["st5_beam_reorder_sents"]
    assert "st5_beam_lm_logprobs_sents" not in plain + ctc and "st5_beam_step_sents_logprobs" not in plain
    # with one: the decoder's launches, the LM's per-row step, the LM term, the beam step on log-probabilities
    lm_ops = ["st5_beam_embed_sents"] + LM_LAYER_ROWS * len(lm.decoder.layers) + ["st5_layernorm_fwd", "st5_gemm_skinny"]
    assert lists["lm"] == plain[:-2] + lm_ops + ["st5_beam_lm_logprobs_sents", "st5_beam_step_sents_logprobs", "st5_beam_reorder_sents"]
    assert lists["lm_ctc"] == plain[:-2] + lm_ops + C.CTC_STEP_SENTS[:2] + ["st5_beam_lm_logprobs_sents"] + C.CTC_STEP_SENTS[2:] + [
        "st5_beam_reorder_sents"]
    for name in ("lm", "lm_ctc"):
        s = lists[name]
        assert s.count("st5_beam_embed_sents") == 2
        assert not [n for n in s if n in ("st5_gemm", "st5_lm_reorder", "st5_lm_decode_attn", "st5_lm_fuse_logprobs", "st5_beam_step_sents",
                                          "st5_beam_lm_logprobs", "st5_beam_embed_step", "st5_lm_decode_attn_dev")]
        admits = lambda head: [n for n in head if n.endswith("_admit")]      # noqa: E731
        assert admits(heads[name]) == admits(heads["plain" if name == "lm" else "ctc"]), "an admission does nothing for the LM"


@pytest.mark.parametrize("scoring", SCORINGS)
def test_generate_gives_the_same_bits_before_and_after_a_stream(cuda, arms, scoring):
    from tests.test_beam_ctc_device_gpu import LENGTHS as RAGGED_LENGTHS
    from tests.test_beam_lm_device_gpu import CONFIGS, RAGGED_KW
    from tests.test_beam_slots_gpu import _ragged_sample
    from speecht5_amd.sequence_generator import SequenceGenerator
    model, d, lm = arms["model"], arms["d"], arms["lm"]
    extra, seed = CONFIGS["ctc" if scoring == "ctc" else "plain"]
    sample = _ragged_sample(cuda, RAGGED_LENGTHS, seed)
    gen = SequenceGenerator([model], d, decode="graph", lm_model=lm, **RAGGED_KW, **extra)
    before = gen.generate([model], sample)
    assert len(_stream(model, d, lm, scoring, 5, arms[scoring], "graph")[1]) == len(arms[scoring])
    after = gen.generate([model], sample)
    assert len(before) == len(after) == 3
    for s, (a, b) in enumerate(zip(before, after)):
        _assert_same_hyps(b, a, f"sentence {s}")


def test_a_tied_output_projection(cuda, arms):
    """The LM of tests/test_beam_lm_device_gpu.py whose output projection is its embedding table, lm_weight 1.0, attention + LM at
    beam 2: every request bit-equal to its reference arm."""
    model, d = arms["model"], arms["d"]
    lm = _tied_lm(cuda, TIED_SEED)
    reqs = arms["att"][:5]
    _, out = _stream(model, d, lm, "att", 2, reqs, "graph", weight=1.0)
    assert sorted(k for k, _ in out) == sorted(k for k, _, _ in reqs)
    for key, hyps in out:
        wav, ml = next((w, m) for k, w, m in reqs if k == key)
        _assert_same_hyps(hyps, _single(model, d, cuda, 2, wav, ml, lm_model=lm, lm_weight=1.0), f"tied {key}")
