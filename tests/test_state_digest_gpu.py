"""st5_state_digest on the GPU against the numpy restatement of its definition (tests/state_digest_reference.py), `==` on every cell:
the sizes {0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 4097} at start offsets {0, 1, 4, 8} (alone: one launch each; all 48 in one launch),
one segment larger than the grid covers in one pass (the grid-stride loop wraps), seven segments of mixed dtypes with an empty one and one
that starts 4 bytes into an allocation, the same call twice, cells pre-filled with garbage, and the malformed arguments."""
import re
import os

import numpy as np
import pytest
import torch

from speecht5_amd import functional as Fn
from tests import state_digest_reference as R

pytestmark = pytest.mark.gpu
ERR_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes_view(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _digest(cuda, tensors, cells=None):
    """One st5_state_digest over `tensors` (device tensors, contiguous) -> list of unsigned ints."""
    nbytes = [t.numel() * t.element_size() for t in tensors]
    prefix = Fn.batch_load_plan(nbytes)
    n = len(tensors)
    tab = torch.tensor([t.data_ptr() for t in tensors] + nbytes + prefix, dtype=torch.int64).to(cuda)
    if cells is None:
        cells = torch.zeros(n, dtype=torch.int64, device=cuda)
    Fn.state_digest(tab[:n], tab[n:2 * n], tab[2 * n:], n, prefix[-1], cells)
    torch.cuda.synchronize()
    return [int(c) & 0xFFFFFFFFFFFFFFFF for c in cells.tolist()]


def _at_offset(cuda, data, off):
    """`data` (numpy uint8) on the device, starting `off` bytes into a 256-byte aligned allocation."""
    buf = torch.zeros(len(data) + off + 16, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 256 == 0
    seg = buf[off:off + len(data)]
    seg.copy_(torch.from_numpy(data))
    return seg


@pytest.mark.parametrize("off", R.OFFSETS)
def test_sizes_and_offsets_one_segment_per_launch(cuda, off):
    for k, n in enumerate(R.SIZES):
        data = R.pattern(n, 10 * k + off)
        assert _digest(cuda, [_at_offset(cuda, data, off)]) == [R.digest(data)], (n, off)


def test_sizes_and_offsets_in_one_launch(cuda):
    datas = [R.pattern(n, 1000 + 7 * i + o) for i, n in enumerate(R.SIZES) for o in R.OFFSETS]
    segs = [_at_offset(cuda, d, o) for d, o in zip(datas, [o for _ in R.SIZES for o in R.OFFSETS])]
    assert _digest(cuda, segs) == [R.digest(d) for d in datas]


def _grid_limits():
    """(grid cap of the accumulate kernel, chunks per workgroup pass, chunk bytes) parsed from the headers the kernel is built from."""
    d = os.path.join(ROOT, "speecht5_amd", "csrc")
    sd, bl = open(os.path.join(d, "state_digest_index.h")).read(), open(os.path.join(d, "batch_load_index.h")).read()
    cap = int(re.search(r"SD_MAX_BLOCKS = (\d+);", sd).group(1))
    chunk, lane, threads = (int(re.search(rf"{k} = (\d+);", bl).group(1)) for k in ("BL_CHUNK", "BL_LANE_BYTES", "BL_THREADS"))
    return cap, threads // (chunk // lane), chunk


def test_grid_stride_loop_wraps(cuda):
    cap, per, chunk = _grid_limits()
    one_pass = cap * per * chunk                   # bytes the full grid covers in one pass of its loop (8 MiB)
    n = 2 * one_pass + 3 * chunk + 5               # two full passes, a partial third, a tail short of a word
    data = np.random.RandomState(4).randint(0, 256, n).astype(np.uint8)
    small = R.pattern(300, 2)
    got = _digest(cuda, [_at_offset(cuda, small, 0), _at_offset(cuda, data, 0), _at_offset(cuda, small, 4)])
    assert got == [R.digest(small), R.digest(data), R.digest(small)]
    assert _digest(cuda, [_at_offset(cuda, data, 4)]) == [R.digest(data)]          # the same bytes on the byte-wise path


def _mixed(cuda):
    g = torch.Generator().manual_seed(9)
    host = [torch.randn(1000, generator=g), torch.randn(333, generator=g).to(torch.bfloat16), torch.randint(-9, 9, (77,), generator=g, dtype=torch.int32),
            torch.randint(0, 256, (4099,), generator=g, dtype=torch.uint8), torch.zeros(0), torch.randn(64, 65, generator=g),
            torch.randn(130, generator=g)]
    dev = [t.to(cuda) for t in host]
    base = torch.zeros(131, dtype=torch.float32, device=cuda)
    base[1:].copy_(host[6])
    dev[6] = base[1:]                              # starts 4 bytes into its allocation
    assert dev[6].data_ptr() % 16 == 4
    return host, dev


def test_mixed_set_repeatable_and_self_initialising(cuda):
    host, dev = _mixed(cuda)
    want = [R.digest(_bytes_view(t).numpy()) for t in host]
    got = _digest(cuda, dev)
    assert got == want
    assert _digest(cuda, dev) == got                                         # the same call twice
    stale = torch.full((len(dev),), -0x0123456789ABCDEF, dtype=torch.int64, device=cuda)
    assert _digest(cuda, dev, cells=stale) == want                           # cells pre-filled with garbage
    assert want[4] == R.digest(b"")


def test_capturable(cuda):
    """No allocation, no host synchronisation: the call records into a graph, and the replay recomputes from the live bytes."""
    host, dev = _mixed(cuda)
    nbytes = [t.numel() * t.element_size() for t in dev]
    prefix = Fn.batch_load_plan(nbytes)
    n = len(dev)
    tab = torch.tensor([t.data_ptr() for t in dev] + nbytes + prefix, dtype=torch.int64).to(cuda)
    cells = torch.zeros(n, dtype=torch.int64, device=cuda)
    s = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        Fn.state_digest(tab[:n], tab[n:2 * n], tab[2 * n:], n, prefix[-1], cells)
    dev[0][17] = 5.0
    host[0][17] = 5.0
    g.replay()
    torch.cuda.synchronize()
    assert [int(c) & 0xFFFFFFFFFFFFFFFF for c in cells.tolist()] == [R.digest(_bytes_view(t).numpy()) for t in host]


def test_argument_errors(cuda):
    from speecht5_amd import hip
    L = hip.lib()
    x = torch.arange(64, dtype=torch.float32, device=cuda)
    tab = torch.tensor([x.data_ptr(), 256, 0, 1], dtype=torch.int64, device=cuda)
    cells = torch.full((1,), 77, dtype=torch.int64, device=cuda)
    a, b, p, o = tab[:1].data_ptr(), tab[1:2].data_ptr(), tab[2:].data_ptr(), cells.data_ptr()
    st = hip.stream()
    assert L.st5_state_digest(a, b, p, -1, 1, o, st) == ERR_ARG
    assert L.st5_state_digest(a, b, p, 1, -1, o, st) == ERR_ARG
    assert L.st5_state_digest(a, b, p, 0, 1, o, st) == ERR_ARG            # chunks and no segment
    for args in ((0, b, p, 1, 1, o), (a, 0, p, 1, 1, o), (a, b, 0, 1, 1, o), (a, b, p, 1, 1, 0)):
        assert L.st5_state_digest(*args, st) == ERR_ARG
    assert L.st5_state_digest(0, 0, 0, 0, 0, 0, st) == 0                  # nothing to do
    torch.cuda.synchronize()
    assert cells.tolist() == [77]                                         # a refused call wrote nothing
    assert L.st5_state_digest(a, b, p, 1, 1, o, st) == 0
    torch.cuda.synchronize()
    assert int(cells[0]) & 0xFFFFFFFFFFFFFFFF == R.digest(x.cpu().numpy())
