// st5_stats_record: the logged scalars of one update -- the criterion's losses, the device-side sample size, code perplexities, the
// squared gradient norm the clip used -- copied into one row of a device ring by ONE launch, the last launch of the update, behind
// Adam (speecht5_amd/train_stats.py StatsRecorder).  Replayed as a node of the captured update it is the only way out for those values:
// the criterion's Python does not run under replay and the scalars live in the graph's private pool.
//
// src [n_cells]: device addresses of the scalars; types [n_cells]: their type codes (train_stats_index.h); ring [rows, 1 + n_cells]:
// 8-byte cells; counter: the number of updates recorded so far.  Row counter % rows gets the stamp `counter` in cell 0 and scalar i,
// widened to fp64 or int64, in cell 1 + i; then the counter becomes counter + 1.  One workgroup: every thread reads the counter, the
// threads loop over the cells, a barrier, one thread stores the new counter.  No atomics, no LDS, plain vector loads and stores; the
// arithmetic (row, cell offset, widening, argument check) is train_stats_index.h, swept on the host.
#include "common.h"
#include "train_stats_index.h"
#include "../../include/speecht5_hip.h"

__global__ void __launch_bounds__(TS_THREADS)
stats_record_kernel(const unsigned long long* __restrict__ src, const int* __restrict__ types, unsigned long long* ring,
                    long long* counter, int rows, int n_cells) {
  const long long c = *counter;
  const long long row = ts_row(c, rows);
  for (int i = threadIdx.x; i < n_cells; i += TS_THREADS) {
    const int type = types[i];
    const unsigned long long a = src[i];
    unsigned long long raw = 0;
    switch (ts_bytes(type)) {
      case 8: raw = *reinterpret_cast<const unsigned long long*>(a); break;
      case 4: raw = *reinterpret_cast<const unsigned int*>(a); break;
      case 2: raw = *reinterpret_cast<const unsigned short*>(a); break;
      case 1: raw = *reinterpret_cast<const unsigned char*>(a); break;
      default: break;
    }
    ring[ts_cell(row, 1 + i, n_cells)] = ts_widen(raw, type);
  }
  if (threadIdx.x == 0) ring[ts_cell(row, 0, n_cells)] = (unsigned long long)c;
  __syncthreads();
  if (threadIdx.x == 0) *counter = c + 1;
}

extern "C" int st5_stats_record(const void* const* src, const int32_t* types, void* ring, int64_t* counter, int32_t rows, int32_t n_cells,
                                void* stream) {
  if (ts_check(rows, n_cells)) return ST5_ERR_ARG;
  if (!src || !types || !ring || !counter) return ST5_ERR_ARG;
  hipLaunchKernelGGL(stats_record_kernel, dim3(1), dim3(TS_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(src), reinterpret_cast<const int*>(types),
                     reinterpret_cast<unsigned long long*>(ring), reinterpret_cast<long long*>(counter), (int)rows, (int)n_cells);
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}
