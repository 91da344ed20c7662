// Index arithmetic and type widening of csrc/train_stats.hip (st5_stats_record: the logged scalars of one update copied into a row of
// a device ring by one launch), as inline functions that compile for the device AND for the host: tests/test_train_stats_cpu.py builds
// this header with the host compiler and sweeps that every cell offset lies inside the ring, that cell 0 is the stamp's, that no two
// cells of a row collide and that every widening is exact.  Nothing here reads memory.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TS_HD __host__ __device__ __forceinline__
#else
#define TS_HD inline
#endif

constexpr int TS_THREADS = 256;       // the one workgroup of a launch
constexpr int TS_MAX_CELLS = 1024;    // compiled cap on the scalars of one update

// type codes of a cell's source (speecht5_amd/train_stats.py TYPE_CODES holds the same numbers)
constexpr int TS_F32 = 0, TS_F64 = 1, TS_BF16 = 2, TS_F16 = 3, TS_I64 = 4, TS_I32 = 5, TS_U8 = 6;

// the argument check of the entry point: 0 when the launch may go ahead
TS_HD int ts_check(long long rows, long long n_cells) { return (rows < 1 || n_cells < 1 || n_cells > TS_MAX_CELLS) ? 1 : 0; }

// the ring row update number `counter` (0, 1, 2, ...) is written to
TS_HD long long ts_row(long long counter, long long rows) {
  const long long r = counter % rows;
  return r < 0 ? r + rows : r;
}

// offset, in 8-byte cells from the ring's base, of cell `cell` of row `row`: cell 0 is the stamp, cell 1 + i scalar i
TS_HD long long ts_cell(long long row, long long cell, long long n_cells) { return row * (1 + n_cells) + cell; }

// bytes read at a source of type `type` (0: unknown type, nothing is read)
TS_HD int ts_bytes(int type) {
  switch (type) {
    case TS_F64: case TS_I64: return 8;
    case TS_F32: case TS_I32: return 4;
    case TS_BF16: case TS_F16: return 2;
    case TS_U8: return 1;
    default: return 0;
  }
}

TS_HD float ts_bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
TS_HD uint64_t ts_f64_bits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

// IEEE half -> float, exact for every bit pattern (subnormals, infinities; a NaN stays a NaN)
TS_HD float ts_f16_f32(uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
  if (e == 0x1Fu) return ts_bits_f32(sign | 0x7F800000u | (m << 13));
  if (e == 0) {
    if (m == 0) return ts_bits_f32(sign);
    int shift = 0;                              // subnormal: m * 2^-24, renormalised
    while (!(m & 0x400u)) { m <<= 1; ++shift; }
    return ts_bits_f32(sign | ((uint32_t)(113 - shift) << 23) | ((m & 0x3FFu) << 13));
  }
  return ts_bits_f32(sign | ((e + 112u) << 23) | (m << 13));
}

// the 8-byte cell for the low ts_bytes(type) bytes `raw` of a source: floating types widened to fp64 (exact for fp32, bf16 and fp16),
// integer and bool types to int64; the host knows each cell's type and reinterprets it
TS_HD uint64_t ts_widen(uint64_t raw, int type) {
  switch (type) {
    case TS_F32: return ts_f64_bits((double)ts_bits_f32((uint32_t)raw));
    case TS_F64: return raw;
    case TS_BF16: return ts_f64_bits((double)ts_bits_f32(((uint32_t)raw & 0xFFFFu) << 16));
    case TS_F16: return ts_f64_bits((double)ts_f16_f32((uint32_t)raw & 0xFFFFu));
    case TS_I64: return raw;
    case TS_I32: return (uint64_t)(int64_t)(int32_t)(uint32_t)raw;
    case TS_U8: return raw & 0xFFu;
    default: return 0;
  }
}
