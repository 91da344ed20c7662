"""functional._JobTable, the job table behind the batched transpose and the batched fp8 quantiser, driven directly with CPU tensors and a
floor of 2 records: records are immutable once appended, the device buffer only grows and outgrown buffers are kept unwritten (a captured
launch may hold their address and reads a prefix), an upload without an append copies nothing, and nothing happens under capture."""
import struct

import pytest
import torch

from speecht5_amd import functional as Fn

CPU = torch.device("cpu")
UNITS = (3, 1, 4)
# the two record formats, with stand-in field values: TrJob {src, dst, rows, cols, tile0, pad} and QuantJob {x, q, s, elems, cols, blk0}
FORMATS = {
    Fn._Bf16Mirror.JOB: lambda i: (lambda start: struct.pack("<qqiiii", 1000 + i, 2000 + i, 64 + i, 128 + i, start, 0)),
    Fn._Fp8Mirror.JOB: lambda i: (lambda start: struct.pack("<QQQqii", (1 << 47) + i, (1 << 46) + i, (1 << 45) + i, 4096 + i, 32 + i, start)),
}
START_AT = {"<qqiiii": 4, "<QQQqii": 5}      # index of the start unit in the unpacked record


@pytest.fixture(params=sorted(FORMATS))
def table(request, monkeypatch):
    """A CPU table of one format with a floor of 2 records; .copies lists the bytes of every copy that went through the table's seam."""
    monkeypatch.setattr(Fn, "_TABLE_FLOOR", 2)
    t = Fn._JobTable("test", CPU, request.param)
    t.fmt, t.rec, t.copies = request.param, FORMATS[request.param], []
    inner = Fn._table_copy

    def counted(dst, src):
        t.copies.append(src.numel())
        inner(dst, src)

    monkeypatch.setattr(Fn, "_table_copy", counted)
    return t


def _bytes(buf, n=None):
    return bytes(buf.numpy()[:n])


def _state(t):
    return (bytes(t.host), t.units, len(t), t.launch_args(), t.dev, None if t.dev is None else _bytes(t.dev), list(t.retired))


def test_records_keep_their_bytes_and_buffers_their_addresses(table):
    R, rec = struct.calcsize(table.fmt), table.rec
    assert R == table.nbytes
    table.append(rec(0), UNITS[0], key="r0")
    table.upload()                                        # first buffer: the floor, 2 records
    first, ptr0 = table.dev, table.launch_args()[0]
    assert first.numel() == 2 * R and table.launch_args() == (first.data_ptr(), 1, 3)
    table.append(rec(1), UNITS[1], key="r1")
    table.upload()                                        # fits: in place
    assert table.dev is first and table.launch_args() == (ptr0, 2, 4) and not table.retired
    assert table.copies == [R, R], "an upload that fits writes the appended suffix only"
    table.upload()                                        # nothing appended: nothing copied
    assert table.copies == [R, R] and table.launch_args() == (ptr0, 2, 4)
    frozen = _bytes(first)

    table.append(rec(2), UNITS[2], key="r2")
    table.upload()                                        # does not fit: grows to max(need, 2 x old) = 4 records
    assert table.dev is not first and table.launch_args()[0] != ptr0 and table.launch_args()[1:] == (3, 8)
    assert table.dev.numel() == 4 * R and table.copies == [R, R, 3 * R]
    assert len(table.retired) == 1 and table.retired[0] is first
    starts = [struct.unpack_from(table.fmt, table.host, R * i)[START_AT[table.fmt]] for i in range(3)]
    assert starts == [0, 3, 4]
    assert bytes(table.host[:2 * R]) == frozen == _bytes(first) == _bytes(table.dev, 2 * R)
    assert bytes(table.host) == b"".join(rec(i)(s) for i, s in enumerate(starts)) == _bytes(table.dev, 3 * R)

    second, ptr1 = table.dev, table.launch_args()[0]
    for i in (3, 4):                                      # two further appends and uploads: one fits, one grows again
        table.append(rec(i), 2, key=f"r{i}")
        table.upload()
    assert [id(b) for b in table.retired] == [id(first), id(second)] and _bytes(first) == frozen, "a retired buffer was written or dropped"
    assert ptr0 == first.data_ptr() and ptr1 == second.data_ptr() and table.launch_args() == (table.dev.data_ptr(), 5, 12)
    assert _bytes(second) == bytes(table.host[:4 * R]) and _bytes(table.dev, 5 * R) == bytes(table.host)
    assert bytes(table.host[:2 * R]) == frozen


def test_nothing_happens_under_capture(table, monkeypatch):
    R, rec = table.nbytes, table.rec
    table.append(rec(0), 3, key="r0")
    table.upload()
    table.append(rec(1), 1, key="r1")
    table.append(rec(2), 4, key="r2")                     # two records pending, and their upload would grow the buffer
    before = _state(table)
    asked = []
    monkeypatch.setattr(Fn, "_capturing", lambda device: asked.append(device) or True)
    with pytest.raises(RuntimeError, match=r"'test'.*append of \('w', 7\).*capturing"):
        table.append(rec(3), 5, key=("w", 7))
    with pytest.raises(RuntimeError, match=r"'test'.*upload of records 1\.\.2.*capturing"):
        table.upload()
    assert _state(table) == before and table.copies == [R] and asked == [CPU, CPU]
    monkeypatch.setattr(Fn, "_capturing", lambda device: False)
    table.upload()
    assert table.launch_args() == (table.dev.data_ptr(), 3, 8) and _bytes(table.dev, 3 * R) == bytes(table.host)


def test_capture_is_not_asked_about_on_the_cpu():
    """torch.cuda.is_current_stream_capturing() raises without a GPU: the predicate must not reach it for a CPU device."""
    assert Fn._capturing(CPU) is False
