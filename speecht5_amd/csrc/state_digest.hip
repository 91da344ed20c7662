// st5_state_digest: one 64-bit digest per segment of a set of device segments (state_digest_index.h has the definition) -- what a
// checkpoint of the update (speecht5_amd/checkpoint.py) is verified with: the device digests its shadow of the state, the host digests
// the bytes that arrived in pinned memory, and the two must agree before anything is written to a file.
//
// A read-only streaming pass with the chunking of st5_batch_load: 256-byte chunks over a grid of at most SD_MAX_BLOCKS workgroups, a
// chunk finds its segment by bisection over the chunk prefix, 16 lanes share a chunk and take 16 bytes = two words each -- one 128-bit
// load when the segment's base is 16-byte aligned, else (and in a segment's tail) byte by byte.  A thread keeps the wrapped sum of its
// summands while its chunks stay inside one segment (the chunks a thread visits ascend, so its segment number never decreases); when a
// 16-lane group moves to another segment, and at the end, the sums are folded with shuffles and one lane adds the result to the
// segment's cell with a 64-bit integer atomic.  Integer addition mod 2^64 commutes: every arrival order gives the same bits.
// Every thread runs the same number of loop iterations and the folds sit behind wave-uniform conditions (__any / __all), so no shuffle
// executes under a partial EXEC mask.  No LDS, no barrier.  Three nodes per call: a memset of the cells, the accumulate kernel, and a
// one-workgroup-per-256-segments kernel that turns each cell's sum into h(sum + n).
#include "common.h"
#include "state_digest_index.h"
#include "../../include/speecht5_hip.h"

typedef unsigned long long sd_u64x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) sd_u64x2* sd_global_vec;
typedef const __attribute__((address_space(1))) unsigned char* sd_global_bytes;

__device__ __forceinline__ unsigned long long sd_fold(unsigned long long v, int width) {
  for (int off = width / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, width);
  return v;
}

__global__ void __launch_bounds__(BL_THREADS)
state_digest_kernel(const unsigned long long* __restrict__ seg, const long long* __restrict__ bytes, const long long* __restrict__ prefix,
                    int n_seg, long long total_chunks, long long iterations, unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x % BL_LANES;
  const long long per = BL_THREADS / BL_LANES;
  unsigned long long acc = 0;
  int cur = -1;                               // the segment `acc` belongs to (-1: none yet)
  // the current segment's table row, kept in registers: segments are long, so the steady state reads nothing but the data
  long long lo = 0, hi = 0, nbytes = 0;       // its chunks are [lo, hi)
  unsigned long long base = 0;
  long long c = (long long)blockIdx.x * per + threadIdx.x / BL_LANES;
  for (long long it = 0; it < iterations; ++it, c += (long long)gridDim.x * per) {
    int s = cur;
    long long b = 0, e = 0;
    if (c < total_chunks) {
      if (c >= hi) {                          // (the chunks a thread visits ascend: c >= lo always holds)
        s = bl_find_leaf(prefix, n_seg, c);
        lo = prefix[s];
        hi = prefix[s + 1];
        nbytes = bytes[s];
        base = seg[s];
      }
      bl_lane_range(c - lo, lane, nbytes, &b, &e);
    }
    // a 16-lane group leaves its segment: fold what it has and hand it over (wave-uniform branch; groups that stay contribute 0)
    const bool leave = s != cur && cur >= 0;
    if (__any(leave)) {
      const unsigned long long sum = sd_fold(leave ? acc : 0ull, BL_LANES);
      if (leave && lane == 0) atomicAdd(out + cur, sum);
      if (leave) acc = 0;
    }
    cur = s;
    if (b < e) {
      if (sd_vector_ok(base, b, e)) {
        const sd_u64x2 q = *(sd_global_vec)(base + b);
        acc += sd_pair_sum(q.x, q.y, b);
      } else {
        acc += sd_lane_sum((sd_global_bytes)base, b, e);
      }
    }
  }
  // the end: one atomic per wave when its four groups ended in the same segment, else one per group
  const int first = __shfl(cur, 0);
  if (__all(cur == first)) {
    const unsigned long long sum = sd_fold(acc, 64);
    if (threadIdx.x % 64 == 0 && cur >= 0) atomicAdd(out + cur, sum);
  } else {
    const unsigned long long sum = sd_fold(acc, BL_LANES);
    if (lane == 0 && cur >= 0) atomicAdd(out + cur, sum);
  }
}

__global__ void __launch_bounds__(256)
state_digest_finish_kernel(const long long* __restrict__ bytes, int n_seg, unsigned long long* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_seg) out[i] = sd_finish(out[i], (unsigned long long)bytes[i]);
}

extern "C" int st5_state_digest(const void* const* seg, const int64_t* bytes, const int64_t* prefix, int32_t n_seg, int64_t total_chunks,
                                uint64_t* out, void* stream) {
  if (n_seg < 0 || total_chunks < 0) return ST5_ERR_ARG;
  if (n_seg == 0) return total_chunks == 0 ? ST5_OK : ST5_ERR_ARG;
  if (!seg || !bytes || !prefix || !out) return ST5_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, sizeof(uint64_t) * (size_t)n_seg, st) != hipSuccess) return ST5_ERR_LAUNCH;
  if (total_chunks > 0) {
    const long long blocks = sd_blocks(total_chunks);
    hipLaunchKernelGGL(state_digest_kernel, dim3((unsigned)blocks), dim3(BL_THREADS), 0, st, reinterpret_cast<const unsigned long long*>(seg),
                       reinterpret_cast<const long long*>(bytes), reinterpret_cast<const long long*>(prefix), (int)n_seg, (long long)total_chunks,
                       sd_iterations(total_chunks, blocks), reinterpret_cast<unsigned long long*>(out));
    HIP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(state_digest_finish_kernel, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const long long*>(bytes), (int)n_seg, reinterpret_cast<unsigned long long*>(out));
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}
