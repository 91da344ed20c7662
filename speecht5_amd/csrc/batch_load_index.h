// Index arithmetic of csrc/batch_load.hip (st5_batch_load: every tensor leaf of an update's micro-batches copied from the incoming
// batch into the graph's static input tensors by one launch), as inline functions that compile for the device AND for the host:
// tests/test_batch_feed_cpu.py builds this header with the host compiler and sweeps, for sets of leaf sizes, that every byte of every
// leaf is covered exactly once and no offset falls outside its leaf.  bl_find_leaf reads the prefix array it is given; nothing else
// here reads memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BL_HD __host__ __device__ __forceinline__
#else
#define BL_HD inline
#endif

constexpr int BL_CHUNK = 256;                        // bytes of one chunk: the unit the grid is spread over
constexpr int BL_LANE_BYTES = 16;                    // bytes one lane moves: one 128-bit load and store when both sides are aligned
constexpr int BL_LANES = BL_CHUNK / BL_LANE_BYTES;   // lanes that share a chunk (a quarter of a wave)
constexpr int BL_THREADS = 256;                      // threads per workgroup = BL_THREADS / BL_LANES chunks per workgroup pass

// chunks of a leaf of `bytes` bytes: a zero-byte leaf contributes none
BL_HD long long bl_chunks(long long bytes) { return bytes <= 0 ? 0 : (bytes + BL_CHUNK - 1) / BL_CHUNK; }

// prefix[0 .. n_leaves]: exclusive prefix of bl_chunks over the leaves (prefix[0] = 0, prefix[n_leaves] = the chunk total).  The leaf
// of chunk c in [0, prefix[n_leaves]) is the one with prefix[i] <= c < prefix[i + 1]: bisection for the first entry above c, at most
// ceil(log2(n_leaves + 1)) probes, every probe inside [0, n_leaves].  Leaves without chunks (equal neighbours) are stepped over.  A c
// outside the range clamps to leaf 0 / n_leaves - 1; bl_lane_range then hands such a lane an empty range.
BL_HD int bl_find_leaf(const long long* prefix, int n_leaves, long long c) {
  int lo = 0, hi = n_leaves;            // the answer + 1 lies in (lo, hi]: prefix[lo] <= c is kept, prefix[hi] > c is kept
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (prefix[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

// the bytes [*begin, *end) of its leaf that `lane` of the leaf's chunk number `k` (= c - prefix[leaf], counted inside the leaf) moves;
// empty (begin == end) behind the leaf's last byte and for a k outside the leaf
BL_HD void bl_lane_range(long long k, int lane, long long bytes, long long* begin, long long* end) {
  long long b = k * BL_CHUNK + (long long)lane * BL_LANE_BYTES;
  if (k < 0 || b > bytes) b = bytes < 0 ? 0 : bytes;
  long long e = b + BL_LANE_BYTES;
  if (e > bytes) e = bytes < b ? b : bytes;
  *begin = b;
  *end = e;
}

// one 128-bit load and store: a whole lane's worth of bytes, both addresses 16-byte aligned (the chunk and lane offsets are
// multiples of 16, so this is the alignment of the two leaf bases); else the lane moves its bytes one by one
BL_HD bool bl_vector_ok(uint64_t src, uint64_t dst, long long begin, long long end) {
  return end - begin == BL_LANE_BYTES && ((src | dst) & 15u) == 0;
}

// workgroups for `chunks` chunks, at most `cap` (the kernel walks the chunks with a grid stride)
BL_HD long long bl_blocks(long long chunks, long long cap) {
  const long long per = BL_THREADS / BL_LANES;
  const long long b = (chunks + per - 1) / per;
  return b > cap ? cap : b;
}
