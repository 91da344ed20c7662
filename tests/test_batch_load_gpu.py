"""st5_batch_load (csrc/batch_load.hip) on the GPU: leaves of mixed dtypes and of the sizes the index sweep of
tests/test_batch_feed_cpu.py covers on the host (0, 1, 15, 16, 17, 255, 256, 257, 4097 bytes, and one of many workgroups), aligned
and misaligned on either side, every destination between two 64-byte canaries."""
import pytest
import torch

from speecht5_amd import functional as Fn

pytestmark = pytest.mark.gpu

# (dtype, elements, source offset in elements, destination offset in bytes behind the front canary)
LEAVES = [
    (torch.bool, 0, 0, 0),            # 0 bytes: no chunk, addresses never read
    (torch.bool, 1, 0, 0),            # 1
    (torch.bool, 15, 1, 0),           # 15, source off by one byte
    (torch.float32, 4, 0, 0),         # 16: one aligned lane
    (torch.bool, 17, 0, 0),           # 17
    (torch.bool, 255, 0, 3),          # 255, destination off by three bytes
    (torch.int64, 32, 0, 0),          # 256: exactly one chunk
    (torch.int64, 32, 1, 0),          # 256, source off by one element (8 bytes)
    (torch.bool, 257, 0, 0),          # 257: a one-byte second chunk
    (torch.bool, 4097, 1, 0),         # 4097: two workgroup passes of chunks, byte path
    (torch.bfloat16, 2049, 0, 0),     # 4098: vector path with a 2-byte tail
    (torch.bfloat16, 2048, 1, 0),     # 4096, source off by one element (2 bytes)
    (torch.float32, 70001, 0, 0),     # 280004 bytes: 1094 chunks, many workgroups
    (torch.float32, 1025, 1, 0),      # 4100, source off by one element (4 bytes)
]


def _draw(dtype, n, g, cuda):
    if dtype == torch.bool:
        return (torch.rand(n, generator=g) > 0.5).to(cuda)
    if dtype == torch.int64:
        return torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g).to(cuda)
    return torch.randn(n, generator=g).to(dtype).to(cuda)


def _sources(seed, cuda):
    g = torch.Generator().manual_seed(seed)
    return [_draw(dt, n + off, g, cuda)[off:] for dt, n, off, _ in LEAVES]


def test_batch_load_copies_every_leaf_and_nothing_else(cuda):
    es = {torch.bool: 1, torch.int64: 8, torch.float32: 4, torch.bfloat16: 2}
    nbytes = [n * es[dt] for dt, n, _, _ in LEAVES]
    assert sorted(set(nbytes) & {0, 1, 15, 16, 17, 255, 256, 257, 4097}) == [0, 1, 15, 16, 17, 255, 256, 257, 4097]
    bufs, dsts = [], []
    for (dt, n, _, doff), nb in zip(LEAVES, nbytes):
        buf = torch.full((64 + doff + nb + 64,), 0xA5, dtype=torch.uint8, device=cuda)
        bufs.append(buf)
        dsts.append(buf[64 + doff:64 + doff + nb])
    prefix = Fn.batch_load_plan(nbytes)
    n = len(LEAVES)
    table = torch.tensor([d.data_ptr() for d in dsts] + nbytes + prefix, dtype=torch.int64).to(cuda)
    col = torch.zeros(n, dtype=torch.int64, device=cuda)
    for seed in (1, 2):                 # the second launch, with a new source column, overwrites every leaf
        srcs = _sources(seed, cuda)
        assert [s.numel() * s.element_size() for s in srcs] == nbytes
        assert any(s.data_ptr() % 16 for s in srcs) and any(s.data_ptr() % 16 == 0 for s in srcs)
        col.copy_(torch.tensor([s.data_ptr() for s in srcs], dtype=torch.int64))
        Fn.batch_load(col, table[:n], table[n:2 * n], table[2 * n:], n, prefix[-1])
        torch.cuda.synchronize()
        for i, ((dt, _, _, doff), s, d, buf, nb) in enumerate(zip(LEAVES, srcs, dsts, bufs, nbytes)):
            assert torch.equal(d, s.view(torch.uint8)), (seed, i)
            if doff % es[dt] == 0:
                assert torch.equal(d.view(dt), s), (seed, i)
            assert bool((buf[:64 + doff] == 0xA5).all()) and bool((buf[64 + doff + nb:] == 0xA5).all()), (seed, i, "canary")
    # a launch without work is accepted and launches nothing; a column of the wrong length is refused before the library sees it
    Fn.batch_load(col, table[:n], table[n:2 * n], table[2 * n:], n, 0)
    with pytest.raises(ValueError):
        Fn.batch_load(col[:3], table[:n], table[n:2 * n], table[2 * n:], n, prefix[-1])
