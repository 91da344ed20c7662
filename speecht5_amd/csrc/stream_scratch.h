// The library's own device scratch (split-K slabs and arenas, LayerNorm partials, fill / scatter / sum-of-squares workspaces), host side
// only: which buffer a stream's launches get, and when a buffer grows.  One rule for all of it, because a captured graph replays
// launches whose kernel arguments are these very addresses:
//   * a stream's state is never handed to another stream (no eviction, however many streams a process goes through);
//   * a buffer that grows leaves its old allocation in place, allocated until the process ends, so whatever was enqueued or
//     captured with the old address stays valid;
//   * a buffer that would have to grow while its stream is capturing does not: the caller gets nullptr (first use and growth happen
//     outside capture);
//   * nothing here frees device memory or waits for the device.
// No HIP header is needed: the device enters through a policy `Dev` with
//   static bool Dev::malloc(void** p, size_t bytes)     true on success
//   static bool Dev::capturing(void* stream)            true when `stream` is being captured (or its state cannot be read)
// (common.h: St5Dev), so tests/test_stream_scratch_cpu.py builds this header with the host compiler and a policy that logs.
#pragma once
#include <cstddef>
#include <deque>
#include <mutex>

// Stream handle -> State, created on first use.  A State* stays valid and keeps its stream for the life of the process (a deque never
// relocates its elements).  The mutex guards lookup and insert only: a state belongs to the thread that drives its stream.  Linear scan:
// the population is bounded by the stream pool of the framework above.
template <typename State>
class PerStream {
 public:
  State* find(void* stream) {
    std::lock_guard<std::mutex> lk(mu_);
    return find_locked(stream);
  }
  State* get(void* stream) {
    std::lock_guard<std::mutex> lk(mu_);
    if (State* st = find_locked(stream)) return st;
    entries_.emplace_back();
    entries_.back().stream = stream;
    return &entries_.back().state;
  }
  // f(stream, state) for every state, in order of creation
  template <typename F>
  void for_each(F f) {
    std::lock_guard<std::mutex> lk(mu_);
    for (Entry& e : entries_) f(e.stream, e.state);
  }

 private:
  struct Entry { void* stream = nullptr; State state{}; };
  State* find_locked(void* stream) {
    for (Entry& e : entries_)
      if (e.stream == stream) return &e.state;
    return nullptr;
  }
  std::mutex mu_;
  std::deque<Entry> entries_;
};

// Grow-only device buffer.  reserve() returns the buffer, at least `need` (> 0) bytes large, or nullptr (allocation failed, or the
// buffer would have to grow while `stream` is capturing; the buffer is then what it was).  Growth goes to max(need, floor, 2 * bytes):
// with every step at least a doubling, all retired allocations together stay smaller than the current one.
template <typename Dev>
struct GrowBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  size_t retired_bytes = 0;    // superseded allocations, left in place

  void* reserve(size_t need, size_t floor, void* stream) {
    if (need <= bytes) return ptr;
    if (Dev::capturing(stream)) return nullptr;
    size_t want = need > floor ? need : floor;
    if (want < 2 * bytes) want = 2 * bytes;
    void* p = nullptr;
    if (!Dev::malloc(&p, want) || !p) return nullptr;
    retired_bytes += bytes;
    ptr = p;
    bytes = want;
    return ptr;
  }
};

// GrowBuf handed out in 256-byte-aligned pieces until reset().  take() never grows: nullptr when the piece does not fit, and the owner
// then folds what it has queued, reset()s, reserve()s and takes again.
template <typename Dev>
struct BumpArena {
  GrowBuf<Dev> buf;
  size_t used = 0;

  static size_t round_up(size_t n) { return (n + 255) & ~(size_t)255; }
  void* take(size_t n) {
    n = round_up(n);
    if (n > buf.bytes - used) return nullptr;
    void* p = static_cast<char*>(buf.ptr) + used;
    used += n;
    return p;
  }
  void reset() { used = 0; }
  // room for one piece of n bytes in an empty arena; a new allocation starts empty (pieces of the retired one stay valid)
  bool reserve(size_t n, size_t floor, void* stream) {
    const void* const old = buf.ptr;
    if (!buf.reserve(round_up(n), floor, stream)) return false;
    if (buf.ptr != old) used = 0;
    return true;
  }
};
