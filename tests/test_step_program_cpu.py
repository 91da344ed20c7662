"""speecht5_amd/step_program.py without a GPU: the layer sequence (append_layers) on fake layers with recording builders that hand out
tags instead of tensors, and the loop (run_steps) in "device" mode with a counting step and a scripted poll."""
from types import SimpleNamespace as NS

import pytest

from speecht5_amd.step_program import append_layers, replay_schedule, run_steps

C, FFN, TMAX, ROWS, H, HD = 8, 24, 5, 3, 2, 4
COUNTER = "counter"


class Recorder:
    """The builders of StepProgram, recording: new() hands out fresh tags, lin / norm / add append one entry each to `log`."""

    def __init__(self):
        self.rows, self.log, self.n = ROWS, [], 0

    def new(self, *shape, dt=None):
        self.n += 1
        return f"buf{self.n}{list(shape)}"

    def lin(self, x, weights, biases, out, **epi):
        self.log.append(("lin", x, [w.name for w in weights], list(biases), out, epi))
        return out

    def norm(self, ln, x, y):
        self.log.append(("norm", ln, x, y))
        return y

    def add(self, op):
        self.log.append(("op", op))


def _linear(name, n=C, k=C):
    return NS(weight=NS(name=name + ".w", shape=(n, k)), bias=name + ".b")


def _attn(name):
    return NS(embed_dim=C, num_heads=H, head_dim=HD, q_proj=_linear(name + ".q"), k_proj=_linear(name + ".k"), v_proj=_linear(name + ".v"),
              out_proj=_linear(name + ".o"))


def _layer(i, cross, normalize_before):
    """normalize_before None: the attribute is missing (as is encoder_attn then): a layer of the LM."""
    layer = NS(self_attn=_attn(f"L{i}.sa"), self_attn_layer_norm=f"L{i}.sa_ln", final_layer_norm=f"L{i}.ff_ln", fc1=_linear(f"L{i}.fc1", FFN, C),
               fc2=_linear(f"L{i}.fc2", C, FFN), act=f"L{i}.act")
    if normalize_before is not None:
        layer.normalize_before = normalize_before
    if cross:
        layer.encoder_attn, layer.encoder_attn_layer_norm = _attn(f"L{i}.ca"), f"L{i}.ca_ln"
    return layer


CONFIGS = {"pre-ln cross": (True, True), "post-ln cross": (True, False), "pre-ln lm": (False, None)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_layer_sequence_order_and_data_flow(name):
    cross, nb_attr = CONFIGS[name]
    nb = nb_attr is not False
    layers = [_layer(i, cross, nb_attr) for i in range(2)]
    caches = ["slots0", "slots1"]
    rec, calls = Recorder(), []
    out = append_layers(rec, "x_in", layers, caches, TMAX, COUNTER, lambda *a: calls.append(("self",) + a),
                        (lambda *a: calls.append(("cross",) + a)) if cross else None, "final_ln")
    pos = [0]
    attn_ops = []      # (the launch, what it must be called with), run after the walk: a late-bound closure shows only then

    def take(kind):
        entry = rec.log[pos[0]]
        pos[0] += 1
        assert entry[0] == kind, (pos[0] - 1, entry)
        return entry[1:]

    def norm(ln, x):
        got_ln, got_x, y = take("norm")
        assert (got_ln, got_x) == (ln, x)
        return y

    def lin(x, names, residual=None, **epi):
        got_x, got_w, got_b, y, got_epi = take("lin")
        assert (got_x, got_w, got_b) == (x, [n + ".w" for n in names], [n + ".b" for n in names])
        assert got_epi == (dict(epi, residual=residual) if residual is not None else epi)
        return y

    def attention(*front, back=()):
        """The launch, and the context buffer: what the out-projection behind it reads."""
        (op,) = take("op")
        ctx = rec.log[pos[0]][1]
        attn_ops.append((op, front + (ctx,) + back))
        return ctx

    def block(ln, x, body):
        """Pre-LN: x + body(LN(x)); post-LN: LN(x + body(x)); body ends in the product that takes the residual x."""
        y = body(norm(ln, x) if nb else x, x)
        return y if nb else norm(ln, y)

    x = "x_in"
    for i, slots in enumerate(caches):
        p = f"L{i}"

        def self_block(h, res):
            q = lin(h, [p + ".sa.q"])
            assert lin(h, [p + ".sa.k", p + ".sa.v"], step=COUNTER, step_stride=2 * C, step_cap=TMAX, out_ld=TMAX * 2 * C) == slots
            return lin(attention("self", q, slots, back=(H, HD)), [p + ".sa.o"], residual=res)

        def cross_block(h, res):
            q = lin(h, [p + ".ca.q"])
            return lin(attention("cross", i, q), [p + ".ca.o"], residual=res)

        def ffn_block(h, res):
            f = lin(h, [p + ".fc1"], act=p + ".act")
            assert f.endswith(str([ROWS, FFN]))
            return lin(f, [p + ".fc2"], residual=res)

        x = block(p + ".sa_ln", x, self_block)
        if cross:
            x = block(p + ".ca_ln", x, cross_block)
        x = block(p + ".ff_ln", x, ffn_block)
    x = norm("final_ln", x)
    assert x == out and pos[0] == len(rec.log)
    for op, want in attn_ops:
        calls.clear()
        op()
        assert calls == [want]
    assert len(attn_ops) == (4 if cross else 2)
    written = [e[4] for e in rec.log if e[0] == "lin"] + [e[3] for e in rec.log if e[0] == "norm"]
    assert len(set(written)) == len(written), "two launches write one buffer"


def test_no_final_norm_returns_the_last_layers_output():
    rec = Recorder()
    out = append_layers(rec, "x_in", [_layer(0, False, True)], ["slots0"], TMAX, COUNTER, lambda *a: None)
    assert rec.log[-1][0] == "lin" and rec.log[-1][4] == out and rec.log[-1][5] == {"residual": rec.log[4][4]}


# ---- the loop ----
POLL_STEPS = 4
CAPS = [1, 2, POLL_STEPS, POLL_STEPS + 1, 3 * POLL_STEPS]


def _run(cap, finished_at=None):
    """run_steps in "device" mode; the poll reports finished at its finished_at-th call (1-based; None: never)."""
    steps, polls = [], []

    def finished():
        polls.append(len(steps))        # (behind which step the host looked)
        return len(polls) == finished_at

    stats = {"polls": 0, "device_steps": 0, "graph_replays": 0}
    at_poll = run_steps(lambda: steps.append(1), cap, "device", POLL_STEPS, finished, stats)
    assert stats == {"polls": len(polls), "device_steps": len(steps), "graph_replays": 0}
    return len(steps), polls, at_poll


@pytest.mark.parametrize("cap", CAPS)
def test_loop_runs_the_schedule_and_reports_that_it_ran_out(cap):
    groups = replay_schedule(cap, POLL_STEPS, cap)
    assert all(n_replay == 0 for _, _, n_replay, _ in groups)
    steps, polls, at_poll = _run(cap)
    assert steps == cap == sum(n for _, n, _, _ in groups)
    assert polls == [first + n - 1 for first, n, _, poll in groups if poll]
    assert polls == [k for k in range(1, cap + 1) if k % POLL_STEPS == 0 and k < cap]      # where the eager loop polls
    assert at_poll is False


@pytest.mark.parametrize("cap", CAPS)
def test_a_finished_poll_stops_the_loop_behind_its_group(cap):
    n_polls = len([g for g in replay_schedule(cap, POLL_STEPS, cap) if g[3]])
    for k in range(1, n_polls + 1):
        steps, polls, at_poll = _run(cap, finished_at=k)
        assert steps == k * POLL_STEPS and polls == [j * POLL_STEPS for j in range(1, k + 1)] and at_poll is True
    steps, _, at_poll = _run(cap, finished_at=n_polls + 1)       # (a poll that never comes)
    assert steps == cap and at_poll is False


def test_a_poll_that_raises_leaves_the_loop():
    steps = []

    def finished():
        raise KeyError("unknown")

    stats = {"polls": 0, "device_steps": 0, "graph_replays": 0}
    with pytest.raises(KeyError):
        run_steps(lambda: steps.append(1), 3 * POLL_STEPS, "device", POLL_STEPS, finished, stats)
    assert len(steps) == POLL_STEPS and stats["polls"] == 1
