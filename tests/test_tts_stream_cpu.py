"""The scheduling decision of the synthesis stream (speecht5_amd/tts_stream.py stream_schedule): host only, hand-checked cases."""
import pytest

from speecht5_amd.step_program import replay_schedule
from speecht5_amd.tts_stream import assign_rows, stream_schedule

ANCHOR = [16, 4, 4, 4, 12, 4, 4, 8, 4]


def _batched_ticks(lengths, rows, poll_steps):
    """The same list in arrival order through batches of `rows` under replay_schedule's stopping rule: a batch runs whole groups
    until the first polled group behind which no row is active, or until the schedule (cap = the batch's longest row) runs out."""
    total = 0
    for i in range(0, len(lengths), rows):
        batch = lengths[i:i + rows]
        cap = max(batch)
        for first, n_eager, n_replay, poll in replay_schedule(cap, poll_steps):
            last = first + n_eager + n_replay - 1
            total += n_eager + n_replay
            if poll and all(n <= last for n in batch):
                break
    return total


def test_anchor_case():
    # poll 0: rows 0 1 2 <- requests 0 1 2.  tick 4: 1, 2 done; rows 1 2 <- 3, 4 (ends 8, 16).  tick 8: 3 done; row 1 <- 5 (12).
    # tick 12: 5 done; row 1 <- 6 (16).  tick 16: rows 0 1 2 = requests 0, 6, 4 done; rows 0 1 <- 7 (24), 8 (20).  tick 20: 8.  tick 24: 7.
    ticks, order, plan = stream_schedule(ANCHOR, 3, 4, with_plan=True)
    assert ticks == 24
    assert order == [1, 2, 3, 5, 0, 6, 4, 8, 7]
    assert plan == [(0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 1, 4), (4, 2, 4), (5, 1, 8), (6, 1, 12), (7, 0, 16), (8, 1, 16)]
    assert stream_schedule(ANCHOR, 3, 4) == (24, order)
    assert _batched_ticks(ANCHOR, 3, 4) == 36


def test_one_row_runs_the_requests_in_turn():
    # 5 steps end at the poll of tick 8, 3 steps at 12, 4 steps (exactly a group) at 16
    assert stream_schedule([5, 3, 4], 1, 4) == (16, [0, 1, 2])
    assert stream_schedule([5, 3, 4], 1, 1) == (12, [0, 1, 2])


def test_more_rows_than_requests():
    # both admitted at poll 0; rows 2 .. 7 stay idle; request 1 ends at tick 4, request 0 at tick 12
    ticks, order, plan = stream_schedule([9, 2], 8, 4, with_plan=True)
    assert (ticks, order) == (12, [1, 0])
    assert plan == [(0, 0, 0), (1, 1, 0)]


def test_empty_iterable():
    assert stream_schedule([], 3, 4) == (0, [])


def test_a_request_that_finishes_exactly_at_a_poll_frees_its_row_there():
    # request 0 takes exactly two groups: found finished at tick 8, not 12, and request 2 starts there
    ticks, order, plan = stream_schedule([8, 8, 1], 2, 4, with_plan=True)
    assert order == [0, 1, 2] and ticks == 12
    assert plan[2] == (2, 0, 8)
    # one step past the poll costs a whole group
    assert stream_schedule([9], 1, 4) == (12, [0])
    assert stream_schedule([8], 1, 4) == (8, [0])


def test_same_poll_completions_come_in_row_order():
    # requests 1 (row 1) and 2 (row 2) end at tick 4; row 0's request 0 ends at tick 8 with request 3 (row 1) and 4 (row 2)
    assert stream_schedule([8, 4, 3, 4, 2], 3, 4) == (8, [1, 2, 0, 3, 4])


def test_a_zero_step_request_still_takes_one_step():
    assert stream_schedule([0], 1, 4) == (4, [0])


def test_assign_rows_and_bad_arguments():
    assert assign_rows([5, 1, 3], 2) == [(1, 0), (3, 1)]
    assert assign_rows([], 4) == [] and assign_rows([2], 0) == []
    with pytest.raises(ValueError, match="rows"):
        stream_schedule([1], 0, 4)
