"""Save and resume (speecht5_amd/checkpoint.py, csrc/state_digest_index.h), without a GPU:
1. csrc/state_digest_index.h compiled with the host compiler into a program that walks segments exactly as csrc/state_digest.hip walks
   them (256-byte chunks, bisection over the prefix, 16 lanes of two words, 16-byte reads where the segment's address allows them) --
   its digests equal tests/state_digest_reference.py for every size in {0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 4097} at start
   offsets {0, 1, 4, 8}, alone and in sets of several segments with empty ones among them, for a grid of one workgroup (the stride
   loop wraps) and for the kernel's own grid.
2. Properties of the definition: the 512 single-bit flips of a 64-byte segment give 512 distinct digests, none the original's; swapped
   words and an appended zero byte change the digest.
3. checkpoint.host_digest equals the reference on the same inputs.
4. File format: a state dictionary of small CPU tensors survives torch.save / torch.load(weights_only=True); load_checkpoint names the
   segment after one byte of `m` is flipped; a write that fails half-way leaves the old file.
5. numpy's global generator, torch's CPU generator and the dropout seed counter round-trip through host_state / set_host_state."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from speecht5_amd import checkpoint
from speecht5_amd import functional as Fn
from tests import state_digest_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "state_digest_index.h"

// one argument per set: "size:offset,size:offset,...".  Segment j of set i holds the bytes of the 64-bit LCG seeded with 100 i + j
// (tests/state_digest_reference.py pattern), starting `offset` bytes into a 64-byte aligned allocation.
static void fill(unsigned char* p, long long n, unsigned long long seed) {
  unsigned long long x = seed * 2862933555777941757ull + 3037000493ull;
  for (long long i = 0; i < n; ++i) { x = x * 6364136223846793005ull + 1442695040888963407ull; p[i] = (unsigned char)(x >> 56); }
}

// the walk of state_digest_kernel on `blocks` workgroups; every byte read lies in [0, bytes[s]) of its segment (checked)
static int walk(const std::vector<unsigned char*>& seg, const std::vector<long long>& bytes, const std::vector<long long>& prefix,
                long long blocks, std::vector<uint64_t>& out) {
  const int n = (int)seg.size();
  const long long total = prefix[n], per = BL_THREADS / BL_LANES, iterations = sd_iterations(total, blocks);
  out.assign(n, 0);
  for (long long blk = 0; blk < blocks; ++blk) for (int t = 0; t < BL_THREADS; ++t) {
    const int lane = t % BL_LANES;
    long long c = blk * per + t / BL_LANES;
    for (long long it = 0; it < iterations; ++it, c += blocks * per) {
      if (c >= total) continue;
      const int s = bl_find_leaf(prefix.data(), n, c);
      long long b, e;
      bl_lane_range(c - prefix[s], lane, bytes[s], &b, &e);
      if (b >= e) continue;
      if (b < 0 || e > bytes[s] || b % 16) return 1;
      if (sd_vector_ok((uint64_t)(uintptr_t)seg[s], b, e)) {
        uint64_t w[2];
        std::memcpy(w, seg[s] + b, 16);
        out[s] += sd_pair_sum(w[0], w[1], b);
      } else {
        out[s] += sd_lane_sum(seg[s], b, e);
      }
    }
  }
  for (int i = 0; i < n; ++i) out[i] = sd_finish(out[i], (uint64_t)bytes[i]);
  return 0;
}

int main(int argc, char** argv) {
  for (int set = 1; set < argc; ++set) {
    std::vector<long long> bytes, offs;
    for (char* tok = std::strtok(argv[set], ","); tok; tok = std::strtok(nullptr, ",")) {
      long long n = 0, o = 0;
      if (std::sscanf(tok, "%lld:%lld", &n, &o) != 2) return 2;
      bytes.push_back(n); offs.push_back(o);
    }
    const int n = (int)bytes.size();
    std::vector<unsigned char*> raw(n), seg(n);
    std::vector<long long> prefix(n + 1, 0);
    for (int j = 0; j < n; ++j) {
      raw[j] = (unsigned char*)std::aligned_alloc(64, (size_t)((bytes[j] + offs[j] + 127) / 64 * 64));
      seg[j] = raw[j] + offs[j];
      fill(seg[j], bytes[j], 100ull * (unsigned long long)(set - 1) + (unsigned long long)j);
      prefix[j + 1] = prefix[j] + bl_chunks(bytes[j]);
    }
    std::vector<uint64_t> one, own;
    if (walk(seg, bytes, prefix, 1, one)) return 3;                                        // one workgroup: the stride loop wraps
    if (walk(seg, bytes, prefix, prefix[n] ? sd_blocks(prefix[n]) : 1, own)) return 3;    // the kernel's grid
    for (int j = 0; j < n; ++j) std::printf("%d %d %016llx %016llx\n", set - 1, j, (unsigned long long)one[j], (unsigned long long)own[j]);
    for (int j = 0; j < n; ++j) std::free(raw[j]);
  }
  return 0;
}
"""

SETS = [[(n, o)] for n in R.SIZES for o in R.OFFSETS] + [
    [(4097, 0), (0, 0), (17, 4), (256, 1), (9, 8)],
    [(0, 0), (0, 4), (5, 1), (0, 0), (300, 4), (0, 8)],
    [(n, R.OFFSETS[i % 4]) for i, n in enumerate(R.SIZES)],
    [(n, R.OFFSETS[(i + 1) % 4]) for i, n in enumerate(reversed(R.SIZES))],
]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_header_digests_equal_the_reference(tmp_path):
    src = tmp_path / "digest.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "digest"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "speecht5_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)] + [",".join(f"{n}:{o}" for n, o in s) for s in SETS], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) == sum(len(s) for s in SETS)
    for i, j, one, own in lines:
        i, j = int(i), int(j)
        want = R.digest(R.pattern(SETS[i][j][0], 100 * i + j))
        assert int(one, 16) == want and int(own, 16) == want, (SETS[i], j, one, own, f"{want:016x}")


def test_every_single_bit_flip_of_64_bytes_is_seen_and_none_collide():
    base = R.pattern(64, 7)
    seen = {R.digest(base)}
    for bit in range(512):
        x = base.copy()
        x[bit // 8] ^= 1 << (bit % 8)
        seen.add(R.digest(x))
    assert len(seen) == 513


def test_position_and_length_are_seen():
    x = R.pattern(64, 3)
    y = x.copy()
    y[0:8], y[8:16] = x[8:16], x[0:8]
    assert R.digest(x) != R.digest(y)
    z = np.zeros(16, dtype=np.uint8)          # (two equal words swapped with a third: only the position term tells)
    z[16 - 8:] = 5
    assert R.digest(z) != R.digest(z[::-1].copy())
    for n in (0, 7, 8, 64):
        assert R.digest(x[:n].tobytes()) != R.digest(x[:n].tobytes() + b"\0")
    assert R.digest(b"") != R.digest(b"\0") != R.digest(b"\0\0")


def test_host_digest_equals_the_reference():
    for k, n in enumerate(R.SIZES + [8 * (1 << 20) + 13]):       # (the last one: more than one numpy pass of host_digest)
        x = R.pattern(n, k) if n < 100000 else np.random.RandomState(1).randint(0, 256, n).astype(np.uint8)
        assert checkpoint.host_digest(x) == R.digest(x), n
        assert checkpoint.host_digest(x.tobytes()) == R.digest(x), n
        for off in R.OFFSETS:
            assert checkpoint.host_digest(torch.from_numpy(np.concatenate([np.zeros(off, np.uint8), x]))[off:]) == R.digest(x), (n, off)
    t = torch.arange(-7, 30, dtype=torch.float32).to(torch.bfloat16)
    assert checkpoint.host_digest(t) == R.digest(t.view(torch.int16).numpy())
    assert checkpoint.host_digest(torch.tensor(3, dtype=torch.int64)) == R.digest(np.array([3], dtype=np.int64))


# ---- file format --------------------------------------------------------------------------------------------------------------------
def _small_state():
    g = torch.Generator().manual_seed(5)
    layout = [["a.weight", 0, 6], ["a.bias", 6, 3], ["b.weight", 64, 10]]
    numel = 80
    pflat = torch.zeros(numel)
    for _, off, n in layout:
        pflat[off:off + n] = torch.randn(n, generator=g)
    segs = {"pflat": pflat, "m": torch.randn(numel, generator=g), "v": torch.rand(numel, generator=g),
            "guard": torch.tensor([1, 0, 0, 4], dtype=torch.int32),
            "model.bn.running_mean": torch.randn(5, generator=g), "model.bn.num_batches_tracked": torch.tensor(4)}
    index = [("a.weight", "a.weight", (2, 3), None), ("a.bias", "a.bias", (3,), None), ("b.weight", "b.weight", (10,), None),
             ("tied.weight", "b.weight", (10,), None), ("bn.running_mean", None, (5,), "model.bn.running_mean"),
             ("bn.num_batches_tracked", None, (), "model.bn.num_batches_tracked")]
    meta = {"layout": layout, "numel": numel, "t": 4, "lr": 1e-3, "betas": [0.9, 0.98], "eps": 1e-6, "weight_decay": 0.01, "clip_norm": 1.0}
    extra = {"format": checkpoint.FORMAT, "num_updates": 4, **checkpoint.host_state(), "batches_pulled": 4, "captures": 0, "skip_run": 0,
             "skip_run_first": -1}
    return checkpoint.assemble(segs, index, meta, extra)


def _equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_state_survives_the_file(tmp_path):
    sd = _small_state()
    assert set(sd) == {"model", "optimizer", "extra_state", "digest"}
    assert set(sd["digest"]) == {"pflat", "m", "v", "guard", "model.bn.running_mean", "model.bn.num_batches_tracked"}
    checkpoint.write_checkpoint(sd, tmp_path / "c.pt")
    assert _equal(sd, torch.load(tmp_path / "c.pt", weights_only=True))
    assert _equal(sd, checkpoint.load_checkpoint(tmp_path / "c.pt"))
    assert sorted(os.listdir(tmp_path)) == ["c.pt"]           # (no temporary file left behind)


@pytest.mark.parametrize("what", ["m", "pflat", "model.bn.running_mean", "guard"])
def test_load_checkpoint_names_the_flipped_segment(tmp_path, what):
    sd = _small_state()
    if what == "m":
        sd["optimizer"]["m"].view(torch.uint8)[13] ^= 1
    elif what == "pflat":
        sd["model"]["a.bias"].view(torch.uint8)[2] ^= 0x80
    elif what == "guard":
        sd["optimizer"]["guard"][0] += 1
    else:
        sd["model"]["bn.running_mean"].view(torch.uint8)[0] ^= 4
    torch.save(sd, tmp_path / "c.pt")
    with pytest.raises(ValueError, match=rf"segment {what.replace('.', chr(92) + '.')} "):
        checkpoint.load_checkpoint(tmp_path / "c.pt")


def test_failed_write_leaves_the_old_file(tmp_path, monkeypatch):
    sd = _small_state()
    path = tmp_path / "c.pt"
    checkpoint.write_checkpoint(sd, path)
    old = path.read_bytes()
    sd["optimizer"]["t"] = 5

    def refuse(*a, **k):
        raise OSError("planted")
    monkeypatch.setattr(os, "replace", refuse)
    with pytest.raises(OSError, match="planted"):
        checkpoint.write_checkpoint(sd, path)
    monkeypatch.undo()
    assert path.read_bytes() == old and sorted(os.listdir(tmp_path)) == ["c.pt"]
    real_save = torch.save

    def half(obj, f, *a, **k):          # (a writer that dies after some bytes reached the temporary file)
        f.write(b"torn")
        raise RuntimeError("planted half-way")
    monkeypatch.setattr(torch, "save", half)
    with pytest.raises(RuntimeError, match="half-way"):
        checkpoint.write_checkpoint(sd, path)
    monkeypatch.setattr(torch, "save", real_save)
    assert path.read_bytes() == old and sorted(os.listdir(tmp_path)) == ["c.pt"]
    assert checkpoint.load_checkpoint(path)["optimizer"]["t"] == 4


# ---- host generators ----------------------------------------------------------------------------------------------------------------
def test_host_generators_round_trip(tmp_path):
    k = 17
    np.random.seed(11)
    torch.manual_seed(11)
    Fn.manual_seed(11)
    try:
        np.random.random(5), np.random.normal(size=3), torch.rand(7), Fn.next_seed()      # (normal: a cached gaussian is part of the state)
        saved = checkpoint.host_state()
        torch.save(saved, tmp_path / "h.pt")

        def draw():
            return (np.random.random(k).tolist() + np.random.normal(size=k).tolist() + np.random.randint(0, 1 << 30, k).tolist(),
                    torch.rand(k).tolist() + torch.randperm(k).tolist(), [Fn.next_seed() for _ in range(k)], Fn._S.counter)
        first = draw()
        np.random.seed(0), torch.manual_seed(0), Fn.manual_seed(999)
        checkpoint.set_host_state(torch.load(tmp_path / "h.pt", weights_only=True))
        assert draw() == first
        assert Fn._S.seed == 11 and Fn._S.counter == 1 + k
    finally:
        Fn.manual_seed(0x5EED)
