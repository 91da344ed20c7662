"""The batch feed of the replayed update, without a GPU:
1. csrc/batch_load_index.h compiled with the host compiler and swept: for sets of leaf sizes (0, 1, 15, 16, 17, 255, 256, 257, 4097
   bytes among them) every byte of every leaf is covered exactly once, no offset falls outside its leaf, the bisection stays inside
   the prefix array -- walked exactly as csrc/batch_load.hip walks (grid stride, 16 lanes per chunk).  Two planted faults (an
   off-by-one prefix, a dropped tail) must be caught by the same sweep.
2. graph.batch_signature / graph.BatchFeed on CPU tensors: what the signature holds, and every refusal by name.
3. graph.ReplaySchedule with a fake source and stub steps: the order of pulls and draws with and without the helper thread, and
   what happens when the source ends."""
import os
import shutil
import subprocess

import pytest
import torch

from speecht5_amd import functional as Fn
from speecht5_amd.graph import BatchFeed, ReplaySchedule, batch_signature, padding_mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- 1 ----
SWEEP = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "batch_load_index.h"
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s (line %d) set=%d leaf=%d chunk=%lld lane=%d\n", #cond, __LINE__, set, leaf, c, lane); return 1; } } while (0)

// the lane's byte range as the kernel takes it; PLANT_DROP_TAIL: a kernel that moves whole 16-byte pieces only
static void lane_range(long long k, int lane, long long bytes, long long* b, long long* e) {
  bl_lane_range(k, lane, bytes, b, e);
#ifdef PLANT_DROP_TAIL
  if (*e - *b != BL_LANE_BYTES) *e = *b;
#endif
}

int main() {
  int set = 0, leaf = 0, lane = 0;
  long long c = 0, moved = 0;
  const long long sizes[] = {0, 1, 15, 16, 17, 255, 256, 257, 4097, 511, 512, 513, 4096, 65536 + 3};
  const int NS = sizeof(sizes) / sizeof(sizes[0]);
  std::vector<std::vector<long long>> sets;
  sets.push_back({});                                          // no leaf at all
  for (int i = 0; i < NS; ++i) sets.push_back({sizes[i]});     // every size alone
  sets.push_back(std::vector<long long>(sizes, sizes + 9));    // the listed sizes, in order
  sets.push_back({4097, 257, 256, 255, 17, 16, 15, 1, 0});     // ... reversed: a zero-byte leaf last
  sets.push_back({0, 0, 5, 0, 0, 300, 0});                     // runs of empty leaves, in front, between and behind
  sets.push_back({0, 0, 0});
  { std::vector<long long> v; unsigned r = 12345u;             // 40 pseudo-random leaves
    for (int i = 0; i < 40; ++i) { r = r * 1664525u + 1013904223u; v.push_back((r >> 8) % 3 == 0 ? 0 : (long long)((r >> 10) % 9000)); }
    sets.push_back(v); }
  for (set = 0; set < (int)sets.size(); ++set) {
    const std::vector<long long>& bytes = sets[set];
    const int n = (int)bytes.size();
    std::vector<long long> prefix(n + 1, 0);
    for (int i = 0; i < n; ++i) prefix[i + 1] = prefix[i] + bl_chunks(bytes[i]);
#ifdef PLANT_PREFIX_OFF_BY_ONE
    if (n >= 2) prefix[n / 2] += 1;                            // a table with one interior prefix entry one chunk too high
#endif
    const long long total = prefix[n];
    std::vector<std::vector<int>> seen(n);
    for (int i = 0; i < n; ++i) seen[i].assign((size_t)bytes[i], 0);
    if (n == 0) { CHECK(total == 0); continue; }
    for (int cap = 1; cap <= 8192; cap *= 64) {                // grids of 1, 64, 4096 workgroups at most
      const long long blocks = bl_blocks(total, cap), per = BL_THREADS / BL_LANES;
      CHECK(blocks <= cap && (total == 0 || blocks >= 1) && (blocks - 1) * per < (total > 0 ? total : 1));
      for (int i = 0; i < n; ++i) std::fill(seen[i].begin(), seen[i].end(), 0);
      for (long long blk = 0; blk < blocks; ++blk) for (int t = 0; t < BL_THREADS; ++t) {
        lane = t % BL_LANES;
        for (c = blk * per + t / BL_LANES; c < total; c += blocks * per) {
          leaf = bl_find_leaf(prefix.data(), n, c);
          CHECK(leaf >= 0 && leaf < n);
          CHECK(prefix[leaf] <= c && c < prefix[leaf + 1]);    // the chunk lies in its leaf, and the leaf is not an empty one
          long long b, e;
          lane_range(c - prefix[leaf], lane, bytes[leaf], &b, &e);
          CHECK(0 <= b && b <= e && e <= bytes[leaf] && e - b <= BL_LANE_BYTES);
          if (bl_vector_ok(0x1000, 0x2000, b, e)) CHECK(e - b == 16 && b % 16 == 0);
          CHECK(!bl_vector_ok(0x1001, 0x2000, b, e) && !bl_vector_ok(0x1000, 0x2008, b, e));
          for (long long i = b; i < e; ++i) { ++seen[leaf][(size_t)i]; ++moved; }
        }
      }
      for (leaf = 0; leaf < n; ++leaf) for (long long i = 0; i < bytes[leaf]; ++i) { c = i; CHECK(seen[leaf][(size_t)i] == 1); }
    }
    // out-of-range chunk numbers never yield a byte range
    for (int i = 0; i < n; ++i) for (lane = 0; lane < BL_LANES; ++lane) {
      long long b, e;
      leaf = i;
      bl_lane_range(bl_chunks(bytes[i]), lane, bytes[i], &b, &e); CHECK(b == e);
      bl_lane_range(-1, lane, bytes[i], &b, &e); CHECK(b == e);
    }
    c = -1; CHECK(bl_find_leaf(prefix.data(), n, -1) >= 0 && bl_find_leaf(prefix.data(), n, -1) < n);
    c = total; CHECK(bl_find_leaf(prefix.data(), n, total + 7) >= 0 && bl_find_leaf(prefix.data(), n, total + 7) < n);
  }
  CHECK(bl_chunks(0) == 0 && bl_chunks(1) == 1 && bl_chunks(256) == 1 && bl_chunks(257) == 2 && bl_chunks(-4) == 0);
  CHECK(bl_chunks(1LL << 40) == (1LL << 32));
  std::printf("OK %lld bytes moved\n", moved);
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
@pytest.mark.parametrize("fault", ["PLANT_PREFIX_OFF_BY_ONE", "PLANT_DROP_TAIL"])
def test_index_header_sweep_catches_planted_faults(tmp_path, fault):
    r = _sweep(tmp_path, "-D" + fault)
    assert r.returncode == 1 and "FAILED" in r.stdout, (fault, r.stdout + r.stderr)


def test_plan_is_the_prefix_of_256_byte_chunks():
    assert Fn.batch_load_plan([]) == [0]
    assert Fn.batch_load_plan([0, 1, 15, 16, 17, 255, 256, 257, 4097]) == [0, 0, 1, 2, 3, 4, 5, 6, 8, 25]
    with pytest.raises(ValueError):
        Fn.batch_load_plan([4, -1])


# ---- 2 ----
def _speech(seed=0, B=2, S=40, lengths=None):
    g = torch.Generator().manual_seed(seed)
    n = list(lengths) if lengths is not None else [S] * B
    return {"id": torch.arange(B), "task_name": "speech_pretrain", "src_lengths": n, "ntokens_list": [7 + seed],
            "net_input": {"source": torch.randn(B, S, generator=g), "padding_mask": torch.arange(S)[None, :] >= torch.tensor(n)[:, None],
                          "prev_output_tokens": torch.randn(B, 3, 4, generator=g), "tgt_lengths": torch.tensor([3] * B)},
            "target_list": [torch.randint(0, 9, (B, 5), generator=g)], "labels": torch.zeros(B, 6), "dec_target_lengths": torch.tensor([6] * B)}


def _text(seed=0, B=3, T=7, ntokens=19):
    g = torch.Generator().manual_seed(100 + seed)
    return {"id": torch.arange(B), "task_name": "text_pretrain", "ntokens": ntokens, "target": torch.randint(4, 30, (B, T), generator=g),
            "net_input": {"src_tokens": torch.randint(4, 30, (B, T), generator=g), "src_lengths": torch.tensor([T] * B),
                          "prev_output_tokens": torch.randint(4, 30, (B, T), generator=g)}}


def test_signature_holds_paths_shapes_dtypes_and_task_name():
    sig = batch_signature([_speech(), _text()])
    assert [s[0] for s in sig] == ["speech_pretrain", "text_pretrain"]
    leaves = dict((p, (shp, dt)) for p, shp, dt in sig[0][1])
    assert leaves["net_input.source"] == ((2, 40), "torch.float32") and leaves["net_input.padding_mask"] == ((2, 40), "torch.bool")
    assert leaves["target_list.0"] == ((2, 5), "torch.int64") and "src_lengths" not in leaves and "task_name" not in leaves
    assert sig == batch_signature([_speech(5), _text(5)])                  # values do not enter
    assert sig != batch_signature([_speech(S=41), _text()]) and sig != batch_signature([_text(), _speech()])
    feed = BatchFeed([_speech(), _text()])
    assert feed.signature == sig and feed.device.type == "cpu"
    assert feed.n_leaves == 13 and feed.prefix[-1] == feed.total_chunks == sum((n + 255) // 256 for n in feed.nbytes)
    assert ("micro_batches[0].net_input.source", 2 * 40 * 4) in [("micro_batches[%d]." % i + ".".join(map(str, k)), n)
                                                                for (i, k), n in zip(feed.paths, feed.nbytes)]


def _refused(feed, batch, *words):
    feed.set_source([batch])
    before = [dict(s) for s in feed.static]
    with pytest.raises(ValueError) as e:
        feed.pull()
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert feed.pulled is None and [dict(s) for s in feed.static] == before      # a refused batch changes nothing


def test_feed_refusals_name_the_path():
    feed = BatchFeed([_speech(), _text()])
    bad = _speech(1)
    bad["net_input"]["source"] = bad["net_input"]["source"][:, :39].contiguous()
    _refused(feed, [bad, _text(1)], "micro_batches[0].net_input.source", "(2, 39)", "(2, 40)")
    bad = _text(1)
    bad["target"] = bad["target"].int()
    _refused(feed, [_speech(1), bad], "micro_batches[1].target", "torch.int32")
    bad = _speech(1)
    del bad["labels"]
    _refused(feed, [bad, _text(1)], "micro_batches[0].labels", "missing")
    bad = _speech(1)
    bad["net_input"]["extra"] = torch.zeros(1)
    _refused(feed, [bad, _text(1)], "micro_batches[0].net_input.extra", "not in the recorded signature")
    _refused(feed, [_text(1), _speech(1)], "micro_batches[0].task_name", "text_pretrain", "speech_pretrain")
    _refused(feed, [_speech(1)], "list of 2 micro-batches")
    bad = _speech(1)
    bad["net_input"]["source"] = bad["net_input"]["source"].to("meta")
    _refused(feed, [bad, _text(1)], "micro_batches[0].net_input.source", "meta")
    # a host value that reaches a captured launch: text_pretrain's ntokens divides the loss
    _refused(feed, [_speech(1), _text(1, ntokens=18)], "micro_batches[1].ntokens", "18", "19")
    # a padding mirror that cannot be had without reading the device
    bad = _speech(1)
    bad["src_lengths"] = [40, 41]
    _refused(feed, [bad, _text(1)], "micro_batches[0].src_lengths")
    # a source that lies inside another static input
    bad = _speech(1)
    big = feed.static[0]["net_input"]["source"].view(-1)
    bad["labels"] = big[4:16].view(2, 6)
    _refused(feed, [bad, _text(1)], "micro_batches[0].labels", "shares memory")


def test_pull_repoints_the_host_side_and_keeps_what_the_step_fixed():
    static = [_speech(), _text()]
    feed = BatchFeed(static)
    nxt = [_speech(3, lengths=[40, 17]), _text(3)]
    nxt[0]["net_input"]["source"] = nxt[0]["net_input"]["source"].t().contiguous().t()       # not contiguous
    feed.set_source([nxt])
    rec = feed.pull()
    assert feed.pulls == 1 and feed.pulled is rec and all(v.is_contiguous() for v in rec.leaves)
    assert rec.ptrs.dtype == torch.int64 and rec.ptrs.tolist() == [v.data_ptr() for v in rec.leaves] and len(rec.leaves) == feed.n_leaves
    i = feed.paths.index((0, ("net_input", "source")))
    assert torch.equal(rec.leaves[i], nxt[0]["net_input"]["source"]) and rec.ptrs[i] != nxt[0]["net_input"]["source"].data_ptr()
    # logging values and the mirror follow the batch; the static tensors are still the recorded ones (the load kernel writes them)
    assert static[0]["src_lengths"] == [40, 17] and static[0]["ntokens_list"] == [10]
    m = static[0]["net_input"]["padding_mask"]._st5_host
    assert m.dtype == torch.bool and m.shape == (2, 40) and m[0].sum() == 0 and m[1, 17:].all() and not m[1, :17].any()
    assert Fn.host_mirror(static[0]["net_input"]["padding_mask"]) is m
    assert static[0]["net_input"]["source"] is feed.dst[i] and not torch.equal(feed.dst[i], nxt[0]["net_input"]["source"])
    with pytest.raises(StopIteration):
        feed.pull()
    assert feed.pulled is rec
    # a mirror the batch carries (the collater's) wins over src_lengths
    carried = _speech(4)
    carried["net_input"]["padding_mask"]._st5_host = torch.ones(2, 40, dtype=torch.bool)
    assert padding_mirror(carried).all() and padding_mirror(_text()) is None
    carried["net_input"]["padding_mask"]._st5_host = torch.ones(2, 39, dtype=torch.bool)
    with pytest.raises(ValueError, match="padding_mask"):
        padding_mirror(carried)


# ---- 3 ----
class _Loop:
    """A replay loop of stubs around ReplaySchedule: the source's pulls and the steps' host draws in the order they happen."""

    def __init__(self, n_batches, prefetch):
        self.events = []
        self.k = 0
        self.draws = 0
        src = iter(range(n_batches))

        def pull():
            v = next(src)
            self.events.append(("pull", v))
            self.k = v

        def produce(slot):
            self.events.append(("draw", self.k))
            self.draws += 1
            self.slot_of[slot] = self.k
        self.slot_of = {}
        self.ran = []
        self.sched = ReplaySchedule(produce, lambda slot: self.events.append(("upload", self.slot_of[slot])), pull=pull, prefetch=prefetch)

    def record(self):                 # what StepGraph.record does around an eagerly run step
        v = self.sched.pull()
        self.events.append(("draw", self.k))
        self.draws += 1
        self.ran.append(self.k)
        return v

    def replay(self):
        used = self.sched.begin()
        self.ran.append(self.slot_of[used])


@pytest.mark.parametrize("prefetch", [False, True])
def test_pull_order_and_end_of_source(prefetch):
    lp = _Loop(5, prefetch)
    lp.record()
    lp.record()
    lp.sched.prime()
    for _ in range(3):
        lp.replay()
    lp.sched.drain()
    # every pulled batch is trained on exactly once, in order; five pulls, five steps' draws -- none for a step that never runs
    assert lp.ran == [0, 1, 2, 3, 4] and lp.draws == 5
    host = [e for e in lp.events if e[0] != "upload"]
    assert host == [(kind, k) for k in range(5) for kind in ("pull", "draw")], host       # pull k, step k's draws, pull k + 1 ...
    assert [e[1] for e in lp.events if e[0] == "upload"] == [2, 3, 4]
    for _ in range(2):                # the source has ended: the following update raises, and nothing more is drawn
        with pytest.raises(StopIteration):
            lp.replay()
    assert lp.draws == 5 and lp.ran == [0, 1, 2, 3, 4]


def test_prefetch_pulls_the_next_batch_during_the_update():
    lp = _Loop(9, True)
    lp.record()
    lp.record()
    lp.sched.prime()
    lp.replay()
    lp.sched.drain()
    # update 2 has run; batch 3 was pulled during it and its host inputs exist
    assert lp.ran == [0, 1, 2] and ("pull", 3) in lp.events and lp.events[-1] == ("draw", 3)
    assert lp.events.index(("pull", 3)) > lp.events.index(("upload", 2))


def test_a_new_source_after_the_end_continues():
    for prefetch in (False, True):
        lp = _Loop(3, prefetch)
        lp.sched.prime()
        lp.replay()
        lp.replay()
        lp.replay()
        with pytest.raises(StopIteration):
            lp.replay()
        src = iter(range(10, 12))
        old = lp.sched.pull

        def pull(src=src, lp=lp):
            v = next(src)
            lp.events.append(("pull", v))
            lp.k = v
        lp.sched.pull = pull
        lp.sched.new_source()
        lp.replay()
        lp.replay()
        lp.sched.drain()
        assert lp.ran == [0, 1, 2, 10, 11] and lp.draws == 5 and old is not pull


def test_without_a_source_the_schedule_is_the_old_one():
    for prefetch in (False, True):
        ev = []
        s = ReplaySchedule(lambda slot: ev.append(("produce", slot)), lambda slot: ev.append(("upload", slot)), prefetch=prefetch,
                           slot_free=lambda slot: ev.append(("free", slot)))
        s.prime()
        for _ in range(3):
            s.begin()
            s.drain()
        if prefetch:      # capture stages slot 0; every replay hands the other pinned image to the helper, then uploads it
            assert ev == [("free", 0), ("produce", 0), ("upload", 0), ("free", 1), ("produce", 1), ("upload", 1), ("free", 0), ("produce", 0),
                          ("upload", 0), ("free", 1), ("produce", 1)], ev
        else:
            assert ev == [("free", 0), ("produce", 0), ("upload", 0)] * 3, ev
