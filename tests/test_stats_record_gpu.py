"""st5_stats_record (csrc/train_stats.hip) on the GPU through functional.stats_record: cells of all seven types at n_cells = 1, 63, 64,
65 and 257 (one thread, just under / exactly / just over a wave, more cells than the workgroup has threads), every source a small
allocation of its own, some at odd element offsets; a ring of 4 rows wrapped twice by 9 launches whose sources change in between;
ring and counter between 64-byte canaries."""
import math
import struct

import pytest
import torch

from speecht5_amd import functional as Fn
from speecht5_amd import hip
from speecht5_amd.train_stats import TYPE_CODES

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.int64, torch.int32, torch.uint8, torch.bool]
ROWS, LAUNCHES, CANARY = 4, 9, 0x5A
SPECIAL = {
    torch.float32: [-0.0, float("inf"), float("-inf"), float("nan"), 2.0 ** -149, 3.4028234663852886e38],
    torch.float64: [-0.0, float("nan"), 1.0 / 3.0, 5e-324],
    torch.bfloat16: [-0.0, float("inf"), float("nan"), 2.0 ** -133],
    torch.float16: [-0.0, float("-inf"), float("nan"), 2.0 ** -24, 65504.0],
    torch.int64: [2 ** 62, -2 ** 62, -1],
    torch.int32: [2 ** 31 - 1, -2 ** 31, -1],
    torch.uint8: [0, 255],
    torch.bool: [True, False],
}


def _value(dtype, g, launch, i):
    sp = SPECIAL[dtype]
    if (i // len(DTYPES) + launch) % 3 == 0:
        return sp[(i // len(DTYPES) + launch) // 3 % len(sp)]
    if dtype.is_floating_point:
        return float(torch.randn((), generator=g)) * 10.0 ** int(torch.randint(-3, 4, (), generator=g))
    if dtype == torch.bool:
        return bool(torch.randint(0, 2, (), generator=g))
    if dtype == torch.uint8:
        return int(torch.randint(0, 256, (), generator=g))
    return int(torch.randint(-2 ** 31, 2 ** 31 - 1, (), generator=g)) * (2 ** 20 + 1 if dtype == torch.int64 else 1)


def _guarded(n_elems, dtype, cuda):
    """A tensor of n_elems between two 64-byte canaries, and the whole buffer."""
    es = torch.empty((), dtype=dtype).element_size()
    buf = torch.full((64 + n_elems * es + 64,), CANARY, dtype=torch.uint8, device=cuda)
    return buf[64:64 + n_elems * es].view(dtype), buf


def _canaries_ok(buf):
    return bool((buf[:64] == CANARY).all()) and bool((buf[-64:] == CANARY).all())


def _cell(dtype, raw):
    """The Python value of an int64 ring cell written for a source of `dtype`."""
    if dtype.is_floating_point:
        return struct.unpack("<d", struct.pack("<q", raw))[0]
    return bool(raw) if dtype == torch.bool else raw


@pytest.mark.parametrize("n_cells", [1, 63, 64, 65, 257])
def test_stats_record_fills_one_row_per_launch_and_nothing_else(cuda, n_cells):
    g = torch.Generator().manual_seed(100 + n_cells)
    dtypes = [DTYPES[i % len(DTYPES)] for i in range(n_cells)]
    # every source an allocation of its own: 1 + off elements, the scalar at element `off` (odd offsets for every third cell)
    offs = [(1 if i % 3 == 1 else 3 if i % 3 == 2 and i % 2 else 0) for i in range(n_cells)]
    holders = [torch.zeros(1 + off, dtype=dt, device=cuda) for dt, off in zip(dtypes, offs)]
    srcs = [h[off:off + 1] for h, off in zip(holders, offs)]
    assert len({s.data_ptr() for s in srcs}) == n_cells and all(s.data_ptr() % s.element_size() == 0 for s in srcs)
    col = torch.tensor([s.data_ptr() for s in srcs], dtype=torch.int64).to(cuda)
    types = torch.tensor([TYPE_CODES[dt] for dt in dtypes], dtype=torch.int32).to(cuda)
    ring, ring_buf = _guarded(ROWS * (1 + n_cells), torch.int64, cuda)
    counter, counter_buf = _guarded(1, torch.int64, cuda)
    ring.fill_(-7)
    counter.zero_()
    want_ring = torch.full((ROWS, 1 + n_cells), -7, dtype=torch.int64)
    for launch in range(LAUNCHES):
        vals = [_value(dt, g, launch, i) for i, dt in enumerate(dtypes)]
        for s, v, dt in zip(srcs, vals, dtypes):
            s.copy_(torch.tensor([v], dtype=dt))
        Fn.stats_record(col, types, ring, counter, ROWS, n_cells)
        torch.cuda.synchronize()
        got = ring.cpu().view(ROWS, 1 + n_cells)
        row = launch % ROWS
        assert int(got[row, 0]) == launch, (launch, int(got[row, 0]))
        for i, (dt, s) in enumerate(zip(dtypes, srcs)):
            ref = s.cpu()[0].item()                       # what the trainer's .item() reads
            cell = _cell(dt, int(got[row, 1 + i]))
            if isinstance(ref, float) and math.isnan(ref):
                assert isinstance(cell, float) and math.isnan(cell), (launch, i, dt, cell)
            else:
                assert type(cell) is type(ref) and cell == ref, (launch, i, dt, cell, ref)
                if isinstance(ref, float):
                    assert math.copysign(1.0, cell) == math.copysign(1.0, ref), (launch, i, dt, "sign of zero")
        want_ring[row] = got[row]
        assert torch.equal(got, want_ring), (launch, "a row other than the launch's own changed")
        assert int(counter.cpu()) == launch + 1
        assert _canaries_ok(ring_buf) and _canaries_ok(counter_buf), (launch, "canary")
    assert [int(v) for v in ring.cpu().view(ROWS, 1 + n_cells)[:, 0]] == [8, 5, 6, 7]      # wrapped twice


def test_stats_record_refuses_bad_sizes_and_writes_nothing(cuda):
    n = 1025
    src = torch.zeros(1, dtype=torch.float32, device=cuda)
    col = torch.full((n,), src.data_ptr(), dtype=torch.int64, device=cuda)
    types = torch.zeros(n, dtype=torch.int32, device=cuda)
    ring, ring_buf = _guarded(4 * (1 + n), torch.int64, cuda)
    counter, counter_buf = _guarded(1, torch.int64, cuda)
    ring.fill_(-7)
    counter.fill_(3)
    for rows, n_cells in ((4, 0), (4, 1025), (0, 1), (4, -1), (-1, 4)):
        with pytest.raises(hip.HipKernelError):
            Fn.stats_record(col, types, ring, counter, rows, n_cells)
    with pytest.raises(ValueError):          # arrays shorter than n_cells are refused before the library sees them
        Fn.stats_record(col[:3], types, ring, counter, 4, 4)
    with pytest.raises(ValueError):
        Fn.stats_record(col, types, ring[:10], counter, 4, 4)
    torch.cuda.synchronize()
    assert bool((ring == -7).all()) and int(counter.cpu()) == 3 and _canaries_ok(ring_buf) and _canaries_ok(counter_buf)
    Fn.stats_record(col, types, ring, counter, 4, 1024)      # the cap itself is accepted
    torch.cuda.synchronize()
    assert int(counter.cpu()) == 4 and int(ring.view(-1)[3 * 1025]) == 3
