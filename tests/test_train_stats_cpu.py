"""The training statistics of the replayed update, without a GPU:
1. csrc/train_stats_index.h compiled with the host compiler and swept: rows in {1, 2, 4, 64}, n_cells in {1, 63, 64, 65, 257, 1024},
   counters 0 .. 3 * rows and one near 2^40, walked exactly as csrc/train_stats.hip walks (one workgroup, threads looping over the
   cells): every cell offset lies inside the ring, cell 0 is the stamp's, no two cells of a row collide, consecutive counters take
   consecutive rows; the widening is exact for fp32, bf16 and fp16 bit patterns (-0.0, the smallest subnormal, +-inf, NaN), int32 min
   and max, int64 +-2^62 and bool.  Two planted faults (a row index off by one, a dropped last cell) must be caught by the same sweep.
2. train_stats.HarvestSchedule with stub copies and events: every update delivered exactly once and in order, no image reused before
   it was harvested, a stale stamp refused.
3. the audit of logged host values under a batch feed (refusal by name) and task.forward_loss(return_log=...)."""
import os
import random
import shutil
import subprocess

import pytest
import torch

from speecht5_amd.train_stats import HarvestSchedule, TYPE_CODES, check_feed_host_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWEEP = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "train_stats_index.h"
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s (line %d) rows=%lld n_cells=%lld counter=%lld cell=%lld\n", #cond, __LINE__, rows, n, c, cell); return 1; } } while (0)

static long long row_of(long long counter, long long rows) {
#ifdef PLANT_ROW_OFF_BY_ONE
  return ts_row(counter, rows) + 1;
#else
  return ts_row(counter, rows);
#endif
}

static double f64(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }

int main() {
  long long rows = 0, n = 0, c = 0, cell = 0, walked = 0;
  const long long all_rows[] = {1, 2, 4, 64}, all_cells[] = {1, 63, 64, 65, 257, 1024};
  for (long long rows_ : all_rows) for (long long n_ : all_cells) {
    rows = rows_; n = n_;
    CHECK(ts_check(rows, n) == 0);
    const long long ring = rows * (1 + n);
    std::vector<long long> counters;
    for (long long k = 0; k <= 3 * rows; ++k) counters.push_back(k);
    counters.push_back((1LL << 40) - 3);
    counters.push_back((1LL << 40) + 5);
    long long prev_row = -1;
    for (size_t ci = 0; ci < counters.size(); ++ci) {
      c = counters[ci];
      const long long row = row_of(c, rows);
      CHECK(row >= 0 && row < rows && row == c % rows);
      if (ci > 0 && counters[ci] == counters[ci - 1] + 1) CHECK(row == (prev_row + 1) % rows);
      prev_row = row;
      std::vector<int> seen((size_t)ring, 0);
      // the kernel's walk: TS_THREADS threads, thread t takes cells t, t + TS_THREADS, ...; thread 0 the stamp
      for (int t = 0; t < TS_THREADS; ++t) {
        long long last = n;
#ifdef PLANT_DROP_LAST_CELL
        last = n - 1;
#endif
        for (long long i = t; i < last; i += TS_THREADS) {
          cell = 1 + i;
          const long long off = ts_cell(row, cell, n);
          CHECK(off >= 0 && off < ring);
          CHECK(off > ts_cell(row, 0, n));
          ++seen[(size_t)off]; ++walked;
        }
        if (t == 0) { cell = 0; const long long off = ts_cell(row, 0, n); CHECK(off >= 0 && off < ring && off == row * (1 + n)); ++seen[(size_t)off]; }
      }
      for (long long off = 0; off < ring; ++off) {
        cell = off;
        const bool mine = off >= row * (1 + n) && off < (row + 1) * (1 + n);
        CHECK(seen[(size_t)off] == (mine ? 1 : 0));        // every cell of the row once, no cell of another row
      }
    }
  }
  rows = n = c = cell = 0;
  // the argument check
  CHECK(ts_check(0, 1) && ts_check(-1, 1) && ts_check(1, 0) && ts_check(1, -1) && ts_check(1, TS_MAX_CELLS + 1) && !ts_check(1, TS_MAX_CELLS));
  CHECK(TS_MAX_CELLS == 1024);
  // bytes per type
  CHECK(ts_bytes(TS_F32) == 4 && ts_bytes(TS_F64) == 8 && ts_bytes(TS_BF16) == 2 && ts_bytes(TS_F16) == 2 && ts_bytes(TS_I64) == 8 &&
        ts_bytes(TS_I32) == 4 && ts_bytes(TS_U8) == 1 && ts_bytes(7) == 0 && ts_bytes(-1) == 0);
  // fp32: special patterns and a stride over all of them, against the compiler's own conversion
  const uint32_t f32s[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007FFFFFu, 0x00800000u, 0x7F7FFFFFu, 0x7F800000u,
                           0xFF800000u, 0x3F800000u, 0xC2F6E979u};
  for (uint32_t u : f32s) { c = u; float f; std::memcpy(&f, &u, 4); const double d = (double)f; uint64_t w; std::memcpy(&w, &d, 8); CHECK(ts_widen(u, TS_F32) == w); }
  for (uint64_t u = 0; u <= 0xFFFFFFFFull; u += 65521) {
    c = (long long)u; float f; const uint32_t v = (uint32_t)u; std::memcpy(&f, &v, 4);
    if (std::isnan(f)) { CHECK(std::isnan(f64(ts_widen(u, TS_F32)))); continue; }
    CHECK(f64(ts_widen(u, TS_F32)) == (double)f && std::signbit(f64(ts_widen(u, TS_F32))) == std::signbit(f));
  }
  CHECK(std::signbit(f64(ts_widen(0x80000000u, TS_F32))) && f64(ts_widen(0x80000000u, TS_F32)) == 0.0);
  CHECK(f64(ts_widen(0x00000001u, TS_F32)) == std::ldexp(1.0, -149));
  CHECK(std::isnan(f64(ts_widen(0x7FC00000u, TS_F32))) && std::isnan(f64(ts_widen(0x7F800001u, TS_F32))));
  // bf16: every pattern (the upper half of an fp32); the upper source bytes are ignored
  for (uint32_t h = 0; h <= 0xFFFFu; ++h) {
    c = h; float f; const uint32_t v = h << 16; std::memcpy(&f, &v, 4);
    if (std::isnan(f)) { CHECK(std::isnan(f64(ts_widen(h, TS_BF16)))); continue; }
    CHECK(f64(ts_widen(h, TS_BF16)) == (double)f && std::signbit(f64(ts_widen(h, TS_BF16))) == std::signbit(f));
    CHECK(ts_widen(h | 0xABCD0000ull, TS_BF16) == ts_widen(h, TS_BF16));
  }
  CHECK(f64(ts_widen(0x0001u, TS_BF16)) == std::ldexp(1.0, -133) && std::isinf(f64(ts_widen(0xFF80u, TS_BF16))));
  // fp16: every pattern against the definition (-1)^s 2^(e-15) (1 + m / 1024), subnormals m 2^-24
  for (uint32_t h = 0; h <= 0xFFFFu; ++h) {
    c = h;
    const int s = h >> 15, e = (h >> 10) & 31, m = h & 1023;
    const double got = f64(ts_widen(h, TS_F16));
    if (e == 31 && m) { CHECK(std::isnan(got)); continue; }
    double want = e == 31 ? std::numeric_limits<double>::infinity() : e == 0 ? std::ldexp((double)m, -24) : std::ldexp(1.0 + m / 1024.0, e - 15);
    if (s) want = -want;
    CHECK(got == want && std::signbit(got) == (s != 0));
  }
  CHECK(f64(ts_widen(0x0001u, TS_F16)) == std::ldexp(1.0, -24) && f64(ts_widen(0x8000u, TS_F16)) == 0.0 && std::signbit(f64(ts_widen(0x8000u, TS_F16))));
  CHECK(f64(ts_widen(0x7C00u, TS_F16)) == std::numeric_limits<double>::infinity() && f64(ts_widen(0xFC00u, TS_F16)) == -std::numeric_limits<double>::infinity());
  // fp64 and the integers
  { const double d = -1.0 / 3.0; uint64_t w; std::memcpy(&w, &d, 8); CHECK(ts_widen(w, TS_F64) == w); }
  CHECK((int64_t)ts_widen(0x80000000u, TS_I32) == -2147483648LL && (int64_t)ts_widen(0x7FFFFFFFu, TS_I32) == 2147483647LL);
  CHECK((int64_t)ts_widen(0xFFFFFFFFu, TS_I32) == -1 && (int64_t)ts_widen(0xDEAD00000005ull, TS_I32) == 5);
  CHECK((int64_t)ts_widen((uint64_t)(1LL << 62), TS_I64) == (1LL << 62) && (int64_t)ts_widen((uint64_t)(-(1LL << 62)), TS_I64) == -(1LL << 62));
  CHECK(ts_widen(0, TS_U8) == 0 && ts_widen(1, TS_U8) == 1 && ts_widen(255, TS_U8) == 255 && ts_widen(0xFF01u, TS_U8) == 1);
  CHECK(ts_widen(12345, 7) == 0);
  std::printf("OK %lld cells walked\n", walked);
  return 0;
}
"""


def _sweep(tmp_path, *defines):
    src = tmp_path / "sweep.cpp"
    src.write_text(SWEEP)
    exe = tmp_path / ("sweep" + "".join(defines).replace("-D", "_"))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *defines, "-I", os.path.join(ROOT, "speecht5_amd", "csrc"), str(src),
                           "-o", str(exe)])
    return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_index_header_sweep_on_the_host(tmp_path):
    r = _sweep(tmp_path)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
@pytest.mark.parametrize("fault", ["PLANT_ROW_OFF_BY_ONE", "PLANT_DROP_LAST_CELL"])
def test_index_header_sweep_catches_planted_faults(tmp_path, fault):
    r = _sweep(tmp_path, "-D" + fault)
    assert r.returncode == 1 and "FAILED" in r.stdout, (fault, r.stdout + r.stderr)


def test_type_codes_match_the_header():
    hdr = open(os.path.join(ROOT, "speecht5_amd", "csrc", "train_stats_index.h")).read()
    import re
    m = re.search(r"TS_F32 = (\d), TS_F64 = (\d), TS_BF16 = (\d), TS_F16 = (\d), TS_I64 = (\d), TS_I32 = (\d), TS_U8 = (\d);", hdr)
    assert m, "the type-code line of train_stats_index.h"
    want = [int(v) for v in m.groups()]
    assert [TYPE_CODES[t] for t in (torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.int64, torch.int32, torch.uint8)] == want
    assert TYPE_CODES[torch.bool] == TYPE_CODES[torch.uint8]


# ---- 2 ----
class _Device:
    """A stand-in for ring, stream and events: record(k) writes update k's row at once; a copy snapshots the ring when it 'executes',
    `delay` updates after it was enqueued (0: at once; many: only when waited for)."""

    def __init__(self, rows, delay, stale=None):
        self.rows, self.delay, self.stale = rows, delay, stale
        self.ring = [(-1, None)] * rows
        self.images = [None, None]
        self.n = 0
        self.copies = []          # [image, enqueued at update, executed, snapshot]
        self.unharvested = set()  # images copied into and not yet read completely
        self.waits = 0
        self.sched = HarvestSchedule(rows, self.copy, self.done, self.wait, self.read)

    def update(self):
        k = self.n
        stamp = k if k != self.stale else k - 1
        self.ring[k % self.rows] = (stamp, f"u{k + 1}")
        self.n += 1
        for c in self.copies:
            if not c[2] and self.n - c[1] > self.delay:
                self._execute(c)
        self.sched.updated()

    def _execute(self, c):
        for d in self.copies:        # stream order: every earlier copy first
            if d is c:
                break
            if not d[2]:
                self._execute(d)
        c[2] = True
        self.images[c[0]] = list(c[3])

    def copy(self, image):
        assert image not in self.unharvested, f"image {image} reused before it was harvested"
        self.unharvested.add(image)
        c = [image, self.n, False, list(self.ring)]    # (the copy is ordered behind update n: it sees the ring as it is now)
        self.copies.append(c)
        if self.delay == 0:
            self._execute(c)
        return c

    def done(self, c):
        return c[2]

    def wait(self, c):
        self.waits += 1
        if not c[2]:
            self._execute(c)

    def read(self, image, row):
        c = self.sched.pending[0]
        assert c[0] == image and c[1][2], "an image is read only once its copy has completed"
        self.unharvested.discard(image)
        return self.images[image][row]


@pytest.mark.parametrize("delay", [0, 1, 10 ** 9], ids=["at_once", "one_update_late", "only_when_waited_for"])
@pytest.mark.parametrize("rows", [2, 4, 5, 64])
def test_harvest_schedule_delivers_every_update_once_and_in_order(rows, delay):
    rnd = random.Random(rows * 7 + min(delay, 3))
    for n_updates in list(range(0, 20)) + [63, 64, 65, 127, 128, 129, 200]:
        dev = _Device(rows, delay)
        got = []
        for _ in range(n_updates):
            dev.update()
            if rnd.random() < 0.3:
                part = dev.sched.harvest()
                assert all(k <= dev.n for k, _ in part)
                got += part
        waits = dev.waits
        got += dev.sched.harvest()          # never waits
        assert dev.waits == waits
        dev.sched.drain()
        got += dev.sched.harvest()
        assert got == [(k, f"u{k}") for k in range(1, n_updates + 1)], (rows, delay, n_updates)
        assert not dev.sched.pending and dev.sched.harvest() == []
        # a copy every rows // 2 updates, into alternating images, plus at most the final one
        every = rows // 2
        assert [c[1] for c in dev.copies][:n_updates // every] == [every * (i + 1) for i in range(n_updates // every)]
        assert len(dev.copies) == n_updates // every + (1 if n_updates % every else 0)
        assert [c[0] for c in dev.copies] == [i % 2 for i in range(len(dev.copies))]


def test_harvest_without_completed_copies_returns_nothing_and_does_not_wait():
    dev = _Device(4, 10 ** 9)
    for _ in range(3):
        dev.update()
    assert dev.sched.harvest() == [] and dev.waits == 0 and len(dev.sched.pending) == 1
    dev.sched.drain()
    assert [k for k, _ in dev.sched.harvest()] == [1, 2, 3]


@pytest.mark.parametrize("rows", [2, 4, 5, 64])
def test_harvest_schedule_refuses_a_stale_stamp(rows):
    dev = _Device(rows, 0, stale=rows + 1)      # update rows + 2 leaves the previous lap's stamp + ... in its row
    with pytest.raises(RuntimeError) as e:
        for _ in range(3 * rows):
            dev.update()
            dev.sched.harvest()
        dev.sched.drain()
    assert f"holds the stamp {rows}" in str(e.value) and f"expects {rows + 1}" in str(e.value), str(e.value)


def test_schedule_refuses_a_ring_of_one_row():
    with pytest.raises(ValueError):
        HarvestSchedule(1, None, None, None, None)


# ---- 3 ----
def test_feed_host_value_audit_refuses_a_free_logged_value_by_name():
    from speecht5_amd.graph import HOST_VALUES_FREE
    check_feed_host_values(["speech_pretrain", "text_pretrain"], HOST_VALUES_FREE)       # today's criteria pass
    free = dict(HOST_VALUES_FREE, text_pretrain=("nsentences", "ntokens"))
    with pytest.raises(ValueError, match="text_pretrain.*ntokens"):
        check_feed_host_values(["speech_pretrain", "text_pretrain"], free)
    with pytest.raises(ValueError, match="my_task"):
        check_feed_host_values(["my_task"], HOST_VALUES_FREE)


def test_forward_loss_default_return_is_unchanged():
    from speecht5_amd.task import SpeechT5Task

    class _M:
        def train(self):
            pass

        def set_num_updates(self, n):
            pass
    loss = torch.tensor(6.0)
    log = {"loss": loss, "ntokens": 3, "nsentences": 2, "sample_size": 3}
    crit = lambda model, sample: (loss, 3, log)
    task = SpeechT5Task.__new__(SpeechT5Task)
    out = task.forward_loss({"task_name": "text_pretrain"}, _M(), crit, 0)
    assert torch.is_tensor(out) and float(out) == 2.0
    out, agg = task.forward_loss({"task_name": "text_pretrain"}, _M(), crit, 0, return_log=True)
    assert float(out) == 2.0 and list(agg) == ["sample_size", "text_pretrain", "ntokens", "nsentences", "loss"]
    assert agg["sample_size"] == 1 and agg["text_pretrain"] is log and agg["ntokens"] == 3 and float(agg["loss"]) == 2.0
