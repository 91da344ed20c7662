"""The transposed copies and fp8 images of the bf16 mirror across a captured refresh (functional.refresh_weight_images): a graph captured
when the job tables held A and B keeps refreshing exactly A and B, from buffers the tables still hold, after a later matrix has outgrown
both tables -- the prefix rule of functional._JobTable.  The refusal under capture is checked on the CPU
(test_weight_image_table_cpu.py): an exception inside a capture is not something to provoke on a device."""
from types import SimpleNamespace

import pytest
import torch

from speecht5_amd import functional as Fn
from speecht5_amd import hip

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
# The smallest shapes that meet every rule of the two launches: whole 64 x 64 transpose tiles in one dimension and a ragged count in
# the other (C: ragged both ways), column counts that are multiples of 32 both ways round (MX blocks), offsets that are multiples of 8.
SHAPES = dict(A=(64, 128), B=(128, 64), C=(96, 160))
OFFSETS = dict(A=0, B=8192, C=16384)
TOTAL = 16384 + 96 * 160


def _values(seed, cuda):
    return torch.randn(TOTAL, generator=torch.Generator().manual_seed(seed)).to(BF).to(cuda)


@pytest.fixture
def mirror(cuda, monkeypatch):
    prev = Fn.compute_dtype()
    uploads = []
    inner = Fn._table_copy
    monkeypatch.setattr(Fn, "_TABLE_FLOOR", 2)
    monkeypatch.setattr(Fn, "_table_copy", lambda dst, src: (uploads.append(src.numel()), inner(dst, src)))
    flat = _values(1, cuda)
    params = [torch.nn.Parameter(torch.zeros(*shp, device=cuda)) for shp in SHAPES.values()]
    try:
        Fn.set_compute_dtype(BF)
        Fn.set_fp8(True)
        Fn.weight_cache.clear()
        Fn.bf16_mirror.attach(flat, params, list(OFFSETS.values()))
        yield SimpleNamespace(flat=flat, uploads=uploads, params=params)
    finally:
        Fn.set_fp8(False)
        Fn.bf16_mirror.__init__()
        Fn.weight_cache.clear()
        Fn.set_compute_dtype(prev)


def _register(flat, name):
    """The transposed copy of matrix `name` and the fp8 images of both views, as the mirrors hand them out."""
    off, (rows, cols) = OFFSETS[name], SHAPES[name]
    W = flat[off:off + rows * cols].view(rows, cols)
    Wt = Fn.bf16_mirror.transposed(off, rows, cols)
    assert Wt is not None and Wt.shape == (cols, rows) and Wt.is_contiguous()
    q, qt = Fn.fp8_mirror.quantised(W), Fn.fp8_mirror.quantised(Wt)
    assert q is not None and qt is not None
    return SimpleNamespace(name=name, Wt=Wt, q=q, qt=qt)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _holds(reg, values):
    """Do the copy and the four images of a registered matrix hold, byte for byte, what `values` (a whole flat buffer) makes them?"""
    off, (rows, cols) = OFFSETS[reg.name], SHAPES[reg.name]
    W = values[off:off + rows * cols].view(rows, cols)
    Wt = W.t().contiguous()
    (q, s), (qt, st) = hip.quant_mxfp8(W), hip.quant_mxfp8(Wt)
    torch.cuda.synchronize()
    return [_same(reg.Wt.view(torch.int16), Wt.view(torch.int16)), _same(reg.q[0], q), _same(reg.q[1], s), _same(reg.qt[0], qt), _same(reg.qt[1], st)]


def _buffers(table):
    return {b.data_ptr() for b in table.retired + [table.dev]}


def test_captured_refresh_keeps_its_jobs_after_the_tables_grew(cuda, mirror):
    old, new = mirror.flat.clone(), _values(2, cuda)
    assert not _same(old, new)
    tr, f8 = Fn.bf16_mirror.table, Fn.fp8_mirror.table
    # 1. A and B: registered (first use produces them), then refreshed by the batched launches
    A, B = _register(mirror.flat, "A"), _register(mirror.flat, "B")
    Fn.refresh_weight_images()
    assert (len(tr), len(f8)) == (2, 4) and len(Fn.bf16_mirror.jobs) == 2 and len(mirror.uploads) == 2
    assert _holds(A, old) == _holds(B, old) == [True] * 5
    captured = (tr.launch_args(), f8.launch_args())
    assert captured[0][1:] == (2, 4) and captured[1][1:] == (4, 4 * 4)     # (tiles: 1 x 2 + 2 x 1; blocks of 2048 elements: 4 per image)
    # 2. the refresh alone, captured on a side stream: nothing is uploaded inside the capture
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        Fn.refresh_weight_images()
    assert len(mirror.uploads) == 2 and (tr.launch_args(), f8.launch_args()) == captured
    # 3. C outgrows both tables (floor: 2 records; the fp8 table held exactly its 4)
    C = _register(mirror.flat, "C")
    Fn.refresh_weight_images()
    assert (len(tr), len(f8)) == (3, 6) and len(tr.retired) == 1 and len(f8.retired) == 1 and len(mirror.uploads) == 4
    assert tr.launch_args()[0] != captured[0][0] and f8.launch_args()[0] != captured[1][0]
    assert _holds(C, old) == [True] * 5
    # 4. new parameters, then the graph
    mirror.flat.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    # 5. the graph refreshed A and B, and only them
    assert _holds(A, new) == _holds(B, new) == [True] * 5
    assert _holds(C, old) == [True] * 5, "a captured refresh reached a job registered after its capture"
    assert not any(_holds(C, new))
    # 6. an eager refresh knows all three
    Fn.refresh_weight_images()
    assert _holds(A, new) == _holds(B, new) == _holds(C, new) == [True] * 5
    assert len(mirror.uploads) == 4, "a refresh with nothing appended uploaded something"
    # 7. what the graph was captured with is still held
    assert captured[0][0] in _buffers(tr) and captured[1][0] in _buffers(f8)
    assert tr.retired[0].data_ptr() == captured[0][0] and f8.retired[0].data_ptr() == captured[1][0]
