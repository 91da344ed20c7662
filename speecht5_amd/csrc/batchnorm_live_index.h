// Row arithmetic of the live-frame BatchNorm entry points (csrc/batchnorm.hip st5_batchnorm_act_*_live) and of the live-frame row
// launches of csrc/elementwise.hip (st5_pad_time_live, st5_zero_rows_live), as inline functions that compile for the device AND for
// the host: tests/test_batchnorm_live_cpu.py builds this header with the host compiler and sweeps it.  Nothing here reads memory.
//
// A [B, Lx, C] activation of a fixed-shape batch holds `live` frames per batch element that the own-length batch would have held too;
// the frames behind them are padding that exists only because the shape is fixed.  `live` is ONE value for the whole batch (the
// reference pads every row of a batch to the same length), read from device memory by every kernel: a captured launch cannot take it
// as an argument.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BNL_HD __host__ __device__ __forceinline__
#else
#define BNL_HD inline
#endif

// the device cell's value brought into [0, Lx]
BNL_HD long long bnl_clamp(long long live, long long Lx) { return live < 0 ? 0 : (live > Lx ? Lx : live); }
// is physical row r of [B * Lx] a live frame?  (live already clamped)
BNL_HD bool bnl_row_live(long long r, long long Lx, long long live) { return r % Lx < live; }
// the number of live rows among `rows` = B * Lx physical rows: the divisor of the statistics
BNL_HD long long bnl_live_rows(long long rows, long long Lx, long long live) { return (rows / Lx) * live; }
