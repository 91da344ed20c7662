"""csrc/stream_scratch.h (the per-stream tables and grow-only buffers behind the library's own device scratch) without a GPU: the header
built with the host compiler against a device policy that mallocs host memory, logs every allocation and has no free at all -- so
"never frees" holds by construction and the program checks instead that every pointer it was ever handed lies in a logged block, and
reads and writes the superseded ones.  Built twice, plain and with -fsanitize=address,undefined (a stand-alone program: nothing is
preloaded).  Two planted faults -- a 16-slot table that hands slot 0 to the 17th stream, a buffer that returns its old pointer after
growing -- must make the same program report FAILED."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
#include "stream_scratch.h"
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

struct Block { char* p; size_t n; };
static std::vector<Block>& g_log = *new std::vector<Block>;                    // every allocation ever made; nothing is ever taken out
static std::vector<const void*>& g_handed = *new std::vector<const void*>;     // every pointer the code under test ever returned
static bool g_capturing = false;
struct HostDev {
  static bool malloc(void** p, size_t n) {
    *p = std::aligned_alloc(256, (n + 255) & ~(size_t)255);   // (device allocations are at least 256-byte aligned)
    if (!*p) return false;
    g_log.push_back({static_cast<char*>(*p), n});
    return true;
  }
  static bool capturing(void*) { return g_capturing; }
};
static bool logged(const void* q) {
  for (const Block& b : g_log)
    if (static_cast<const char*>(q) >= b.p && static_cast<const char*>(q) < b.p + b.n) return true;
  return false;
}
static void* handed(void* p) { if (p) g_handed.push_back(p); return p; }
static void fill(void* p, size_t n, int v) { std::memset(p, v, n); }
static bool holds(const void* p, size_t n, int v) {
  for (size_t i = 0; i < n; ++i) if (static_cast<const unsigned char*>(p)[i] != (unsigned char)v) return false;
  return true;
}

#ifdef PLANT_REUSE_SLOT0
// the table this header replaces, in small: 16 slots, and the 17th stream is handed slot 0
template <typename State> struct Table {
  void* owner[16] = {}; State st[16] = {}; int n = 0;
  State* find(void* s) { for (int i = 0; i < n; ++i) if (owner[i] == s) return &st[i]; return nullptr; }
  State* get(void* s) { if (State* p = find(s)) return p; const int i = n < 16 ? n++ : 0; owner[i] = s; return &st[i]; }
  template <typename F> void for_each(F f) { for (int i = 0; i < n; ++i) f(owner[i], st[i]); }
};
#else
template <typename State> using Table = PerStream<State>;
#endif

struct Buf : GrowBuf<HostDev> {
  void* reserve(size_t need, size_t floor, void* stream) {
    void* const old = ptr;
    void* p = GrowBuf<HostDev>::reserve(need, floor, stream);
#ifdef PLANT_STALE_POINTER
    if (p && old && p != old) p = old;     // grown, but the caller still gets the superseded block
#endif
    (void)old;
    return handed(p);
  }
};
static size_t log_bytes_before_last(size_t from) { size_t s = 0; for (size_t i = from; i + 1 < g_log.size(); ++i) s += g_log[i].n; return s; }

struct St { int tag = 0; };
static void* handle(int i) { return i == 0 ? nullptr : reinterpret_cast<void*>((uintptr_t)0x7f0000001000ull + 64u * (unsigned)i); }   // (the null stream is a stream)

static int per_stream() {
  const int N = 100;
  Table<St> t;
  std::vector<St*> first(N);
  CHECK(t.find(handle(0)) == nullptr);
  for (int i = 0; i < N; ++i) {
    CHECK(t.find(handle(i)) == nullptr);
    first[i] = t.get(handle(i));
    CHECK(first[i] != nullptr && first[i]->tag == 0);        // a state of its own, fresh
    first[i]->tag = i + 1;
    for (int j = i; j >= 0; j -= 3) {                        // interleaved gets never move or reassign an earlier state
      CHECK(t.get(handle(j)) == first[j] && first[j]->tag == j + 1);
      CHECK(t.find(handle(j)) == first[j]);
    }
  }
  CHECK(std::set<St*>(first.begin(), first.end()).size() == (size_t)N);
  for (int i = 0; i < N; ++i) CHECK(t.find(handle(i)) == first[i] && first[i]->tag == i + 1);
  CHECK(t.find(handle(N + 5)) == nullptr && t.find(reinterpret_cast<void*>((uintptr_t)8)) == nullptr);
  int seen = 0, in_order = 1;
  t.for_each([&](void* s, St& st) { in_order &= (s == handle(seen) && &st == first[seen] && st.tag == seen + 1); ++seen; });
  CHECK(seen == N && in_order);                              // find of an unknown handle created nothing
  return 0;
}

static int grow_buf() {
  Buf b;
  void* const s = handle(1);
  const size_t log0 = g_log.size();
  char* p0 = static_cast<char*>(b.reserve(100, 4096, s));
  CHECK(p0 && g_log.size() == log0 + 1 && g_log.back().n == 4096 && g_log.back().p == p0 && b.bytes == 4096 && b.retired_bytes == 0);
  fill(p0, 4096, 0xA1);
  CHECK(b.reserve(4096, 4096, s) == p0 && b.reserve(1, 1 << 20, s) == p0 && g_log.size() == log0 + 1);   // no growth: same pointer, no allocation
  // growth: exactly one block of max(need, floor, 2 * old); the superseded block stays readable and writable
  const struct { size_t need, floor, want; } steps[] = {
      {4097, 4096, 8192},                 // the doubling decides
      {100000, 4096, 100000},             // the need decides
      {100001, 1 << 20, 1 << 20},         // the floor decides
      {(1 << 20) + 1, 4096, 2 << 20}};
  std::vector<char*> olds{p0};
  for (const auto& st : steps) {
    const size_t n_log = g_log.size(), old_bytes = b.bytes;
    char* p = static_cast<char*>(b.reserve(st.need, st.floor, s));
    CHECK(p && g_log.size() == n_log + 1 && g_log.back().n == st.want);
    CHECK(p == g_log.back().p && p == b.ptr && b.bytes == st.want);          // the NEW block is what the caller gets
    CHECK(b.retired_bytes == log_bytes_before_last(log0) && b.retired_bytes < b.bytes);
    fill(p, st.want, 0xA1 + (int)olds.size());
    for (size_t i = 0; i < olds.size(); ++i) CHECK(holds(olds[i], 64, 0xA1 + (int)i));
    fill(olds.back(), old_bytes, 0xA1 + (int)olds.size() - 1);               // (writable: the sanitizer build judges)
    CHECK(b.reserve(st.need, st.floor, s) == p && b.reserve(1, 0, s) == p && g_log.size() == n_log + 1);
    olds.push_back(p);
  }
  return 0;
}

static int capture() {
  void* const s = handle(2);
  Buf fresh, used;
  char* p = static_cast<char*>(used.reserve(1000, 4096, s));
  CHECK(p);
  const size_t n_log = g_log.size();
  g_capturing = true;
  CHECK(fresh.reserve(1, 4096, s) == nullptr && fresh.ptr == nullptr && fresh.bytes == 0);       // first use under capture: refused
  CHECK(used.reserve(4096, 4096, s) == p);                                                       // fits: served
  CHECK(used.reserve(4097, 4096, s) == nullptr && used.ptr == p && used.bytes == 4096 && used.retired_bytes == 0);
  CHECK(g_log.size() == n_log);                                                                  // ... and nothing was allocated
  BumpArena<HostDev> a;
  CHECK(!a.reserve(100, 4096, s) && a.take(100) == nullptr && g_log.size() == n_log);
  g_capturing = false;
  CHECK(used.reserve(4097, 4096, s) != nullptr && used.bytes == 8192 && fresh.reserve(1, 4096, s) != nullptr);
  return 0;
}

static int bump_arena() {
  void* const s = handle(3);
  BumpArena<HostDev> a;
  CHECK(a.take(1) == nullptr);                                   // nothing reserved yet
  CHECK(a.reserve(1000, 4096, s) && g_log.back().n == 4096);
  char* const base = static_cast<char*>(a.buf.ptr);
  const size_t sizes[] = {1, 300, 256, 255, 1024};               // -> 256, 512, 256, 256, 1024 bytes
  const size_t offs[] = {0, 256, 768, 1024, 1280};
  std::vector<char*> got;
  for (int i = 0; i < 5; ++i) {
    char* p = static_cast<char*>(handed(a.take(sizes[i])));
    CHECK(p == base + offs[i] && (uintptr_t)p % 256 == 0);       // aligned, and in front of it exactly the rounded earlier pieces: disjoint
    fill(p, sizes[i], 0x10 + i);
    got.push_back(p);
  }
  for (int i = 0; i < 5; ++i) CHECK(holds(got[i], sizes[i], 0x10 + i));
  CHECK(a.used == 2304 && a.take(1793) == nullptr && a.used == 2304);   // full for this piece: nullptr, nothing taken
  CHECK(handed(a.take(1792)) == base + 2304 && a.take(1) == nullptr);   // ... the exact remainder fits
  a.reset();
  CHECK(handed(a.take(7)) == base);                              // the same first pointer after a reset
  // a piece larger than the arena: take refuses, reserve grows to max(10240, 4096, 2 * 4096), earlier pieces stay valid
  const size_t n_log = g_log.size();
  CHECK(a.take(10000) == nullptr && a.reserve(10000, 4096, s) && g_log.size() == n_log + 1 && g_log.back().n == 10240);
  char* big = static_cast<char*>(handed(a.take(10000)));
  CHECK(big == a.buf.ptr && big != base && a.take(1) == nullptr);
  fill(big, 10000, 0x77);
  for (int i = 1; i < 5; ++i) CHECK(holds(got[i], sizes[i], 0x10 + i));
  fill(base, 4096, 0x55);
  CHECK(a.reserve(10000, 4096, s) && a.used == 10240 && g_log.size() == n_log + 1);   // enough already: nothing moves, nothing is reset
  CHECK(a.buf.retired_bytes == 4096 && a.buf.retired_bytes < a.buf.bytes);
  return 0;
}

int main() {
  if (per_stream() || grow_buf() || capture() || bump_arena()) return 1;
  for (const void* p : g_handed) CHECK(logged(p));               // whatever was ever handed out is still allocated
  std::printf("OK %zu allocations, %zu pointers handed out\n", g_log.size(), g_handed.size());
  return 0;
}
"""


def _run(tmp_path, *flags):
    src = tmp_path / "stream_scratch_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / ("main" + "".join(flags).replace("-D", "_").replace("-fsanitize=", "_").replace(",", "_"))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "speecht5_amd", "csrc"), str(src),
                           "-o", str(exe)])
    return subprocess.run([str(exe)], capture_output=True, text=True)


needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")


@needs_gxx
@pytest.mark.parametrize("sanitize", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_tables_and_buffers_on_the_host(tmp_path, sanitize):
    r = _run(tmp_path, *sanitize)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


@needs_gxx
@pytest.mark.parametrize("fault", ["PLANT_REUSE_SLOT0", "PLANT_STALE_POINTER"])
def test_planted_faults_are_caught(tmp_path, fault):
    r = _run(tmp_path, "-D" + fault)
    assert r.returncode == 1 and "FAILED" in r.stdout, (fault, r.stdout + r.stderr)
