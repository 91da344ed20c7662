// st5_batch_load: the tensor leaves of an update's micro-batches, copied from the incoming batch into the static input tensors of
// the captured step by ONE launch -- the first node of the replayed update (speecht5_amd/graph.py BatchFeed).  At the benched shape
// this is ~6 MB in ~15 leaves: the cost is launch and memory latency, not bandwidth, and one launch per leaf in front of a replay
// is what HostStaging.pack() removed for the staged inputs (0.3-0.4 ms of idle GPU for 55 blits).
//
// Descriptor table (device memory, written once when the feed is built): per leaf a destination address, a byte count and the
// exclusive prefix of its 256-byte chunks.  The source addresses are a column of their own: the only device values that change
// between two updates; the host checks device, dtype, shape and contiguity of every incoming leaf before it writes an address.
// Chunks are spread over the grid (grid stride); a chunk finds its leaf by bisection over the prefix, bounded by the leaf count
// (batch_load_index.h, swept on the host); 16 lanes share a chunk and move 16 bytes each -- one 128-bit load and store when source
// and destination are both 16-byte aligned, else byte by byte, as is a leaf's tail.  No atomics, no LDS.
#include "common.h"
#include "batch_load_index.h"
#include "../../include/speecht5_hip.h"

__global__ void __launch_bounds__(BL_THREADS)
batch_load_kernel(const unsigned long long* __restrict__ src, const unsigned long long* __restrict__ dst, const long long* __restrict__ bytes,
                  const long long* __restrict__ prefix, int n_leaves, long long total_chunks) {
  const int lane = threadIdx.x % BL_LANES;
  const long long per = BL_THREADS / BL_LANES;
  for (long long c = (long long)blockIdx.x * per + threadIdx.x / BL_LANES; c < total_chunks; c += (long long)gridDim.x * per) {
    const int leaf = bl_find_leaf(prefix, n_leaves, c);
    const long long n = bytes[leaf];
    long long b, e;
    bl_lane_range(c - prefix[leaf], lane, n, &b, &e);
    if (b >= e) continue;
    const unsigned long long s = src[leaf], d = dst[leaf];
    if (bl_vector_ok(s, d, b, e)) {
      *reinterpret_cast<uint4*>(d + b) = *reinterpret_cast<const uint4*>(s + b);
    } else {
      const unsigned char* sp = reinterpret_cast<const unsigned char*>(s);
      unsigned char* dp = reinterpret_cast<unsigned char*>(d);
      for (long long i = b; i < e; ++i) dp[i] = sp[i];
    }
  }
}

extern "C" int st5_batch_load(const void* const* src, const void* const* dst, const int64_t* bytes, const int64_t* prefix, int32_t n_leaves,
                              int64_t total_chunks, void* stream) {
  if (n_leaves < 0 || total_chunks < 0) return ST5_ERR_ARG;
  if (n_leaves == 0 || total_chunks == 0) return total_chunks == 0 ? ST5_OK : ST5_ERR_ARG;
  if (!src || !dst || !bytes || !prefix) return ST5_ERR_ARG;
  const long long blocks = bl_blocks(total_chunks, 8192);
  hipLaunchKernelGGL(batch_load_kernel, dim3((unsigned)blocks), dim3(BL_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(src), reinterpret_cast<const unsigned long long*>(dst),
                     reinterpret_cast<const long long*>(bytes), reinterpret_cast<const long long*>(prefix), (int)n_leaves, (long long)total_chunks);
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}
