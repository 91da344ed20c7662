"""CPU checks of the graph-replayed TTS decode: the replay schedule against the eager loop's control flow, and the fp64 restatement
of the skinny-M GEMM (the reference of tests/test_tts_graph_gpu.py) against torch.nn.functional.linear compositions."""
import pytest
import torch

from tests import tts_graph_reference as R

POLL = 8


def _walk(groups, stop_at_poll=None):
    steps, polls, eager, replays = [], [], [], []
    for first, n_eager, n_replay, poll in groups:
        assert n_eager >= 0 and n_replay >= 0 and n_eager + n_replay >= 1
        assert first == (steps[-1] + 1 if steps else 1)
        for i in range(n_eager + n_replay):
            steps.append(first + i)
            (eager if i < n_eager else replays).append(first + i)
        if poll:
            polls.append(steps[-1])
            if stop_at_poll is not None and len(polls) == stop_at_poll:
                break
    return steps, polls, eager, replays


@pytest.mark.parametrize("cap", range(1, 41))
def test_replay_schedule_walks_the_eager_loop(cap):
    from speecht5_amd.tts_graph import GRAPH_WARMUP_STEPS, replay_schedule
    groups = replay_schedule(cap, POLL)
    steps, polls, eager, replays = _walk(groups)
    want_steps, want_polls = R.eager_loop(cap, POLL)
    assert steps == want_steps == list(range(1, cap + 1))
    assert polls == want_polls == [i for i in range(1, cap + 1) if i % POLL == 0 and i < cap]
    assert max(steps) <= cap
    assert eager == list(range(1, min(GRAPH_WARMUP_STEPS, cap) + 1)), "step 1 runs kernel by kernel in front of the capture"
    assert all(n_eager + n_replay <= POLL for _, n_eager, n_replay, _ in groups), "never more than a poll interval between two polls"
    for p in range(1, len(want_polls) + 1):
        got = _walk(groups, stop_at_poll=p)
        want = R.eager_loop(cap, POLL, stop_at_poll=p)
        assert got[0] == want[0] and got[1] == want[1]
    # the all-eager form ("device") covers the same steps and polls without a replay
    s2, p2, e2, r2 = _walk(replay_schedule(cap, POLL, eager_steps=cap))
    assert s2 == want_steps and p2 == want_polls and r2 == [] and e2 == want_steps


def test_unknown_decode_mode_is_a_value_error():
    from speecht5_amd.speecht5 import T5TransformerModel
    with pytest.raises(ValueError, match="decode"):
        T5TransformerModel._decode_rows_mode(object(), "fast", None, None, None, None, True)


@pytest.mark.parametrize("N,K", [(256, 80), (162, 768), (768, 1280)])
def test_fp64_restatement_matches_linear_compositions(N, K):
    g = torch.Generator().manual_seed(N + K)
    F = torch.nn.functional
    x = torch.randn(5, K, generator=g, dtype=torch.float64)
    w = torch.randn(N, K, generator=g, dtype=torch.float64) / K ** 0.5
    b = torch.randn(N, generator=g, dtype=torch.float64)
    res = torch.randn(5, N, generator=g, dtype=torch.float64)
    tol = dict(rtol=0, atol=1e-12)
    torch.testing.assert_close(R.skinny_gemm(x, [w]), F.linear(x, w), **tol)
    torch.testing.assert_close(R.skinny_gemm(x, [w], [b]), F.linear(x, w, b), **tol)
    torch.testing.assert_close(R.skinny_gemm(x, [w], [b], act=R.ACT_RELU), F.relu(F.linear(x, w, b)), **tol)
    torch.testing.assert_close(R.skinny_gemm(x, [w], [b], act=R.ACT_GELU), F.gelu(F.linear(x, w, b)), **tol)
    torch.testing.assert_close(R.skinny_gemm(x, [w], [b], act=R.ACT_TANH), torch.tanh(F.linear(x, w, b)), **tol)
    torch.testing.assert_close(R.skinny_gemm(x, [w], [b], residual=res), F.linear(x, w, b) + res, **tol)
    h = N // 2
    stacked = torch.cat([F.linear(x, w[:h], b[:h]), F.linear(x, w[h:], b[h:])], dim=1)
    torch.testing.assert_close(R.skinny_gemm(x, [w[:h], w[h:]], [b[:h], b[h:]]), stacked, **tol)


def test_ulp_at_scale():
    assert R.ulp_at_scale(torch.tensor([1.5]), torch.float32) == 2.0 ** -23
    assert R.ulp_at_scale(torch.tensor([-5.0, 1.0]), torch.bfloat16) == 2.0 ** (2 - 7)
