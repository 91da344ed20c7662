// Index arithmetic of st5_ctc_pack_rows (csrc/ctc_loss.hip: the CTC labels of a right-padded target batch packed per row, on the
// device), as inline functions that compile for the device AND for the host: tools/ctc_pack_sweep.cpp builds this header with the host
// compiler (address and undefined-behaviour sanitizers on) and walks rows exactly as the kernel walks them -- 64 columns per chunk, one
// ballot per chunk, a running base -- checking that the kept entries land in order from column 0, that every column of the output row
// is written exactly once (a kept entry or the tail fill) and that no destination leaves the row.  Nothing here reads memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CP_HD __host__ __device__ __forceinline__
#else
#define CP_HD inline
#endif

constexpr int CP_WAVE = 64;           // columns per chunk: one lane each, one ballot per chunk
constexpr int CP_THREADS = 1024;      // the one workgroup of a launch: CP_THREADS / CP_WAVE waves, rows dealt out wave by wave
constexpr int CP_WAVES = CP_THREADS / CP_WAVE;
constexpr int CP_AHEAD = 4;           // chunks a wave loads before it compacts the first of them (the loads are independent)

// the argument check of the entry point: 0 when the launch may go ahead (B * L elements are indexed with long long)
CP_HD int cp_check(long long B, long long L) { return (B < 0 || L < 0 || B > 0x7fffffffLL || L > 0x7fffffffLL) ? 1 : 0; }

// chunks of CP_WAVE columns that cover a row of L columns
CP_HD long long cp_chunks(long long L) { return L <= 0 ? 0 : (L + CP_WAVE - 1) / CP_WAVE; }

// the column lane `lane` reads in chunk `chunk` (the chunk base plus the lane); it holds an entry only when < L
CP_HD long long cp_column(long long chunk, int lane) { return chunk * CP_WAVE + lane; }

// offset of row b's first entry in `packed` (and the value of offsets[b]): rows keep their stride, nothing is made contiguous
CP_HD long long cp_offset(long long b, long long L) { return b * L; }

// an entry is kept when it is neither the padding symbol nor the end-of-sentence symbol
CP_HD int cp_keep(long long v, long long pad, long long eos) { return (v != pad && v != eos) ? 1 : 0; }

CP_HD int cp_popcount(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(m);
#else
  return __builtin_popcountll(m);
#endif
}

// the lane's destination column inside the row: the running base (kept entries of the chunks in front) plus the kept entries of the
// lanes in front of it in this chunk (EXCLUSIVE prefix popcount of the chunk's ballot): stable, so the order of the row is kept
CP_HD long long cp_lane_dest(long long base, uint64_t ballot, int lane) {
  const uint64_t below = lane <= 0 ? 0ull : (lane >= 64 ? ~0ull : ((1ull << lane) - 1ull));
  return base + cp_popcount(ballot & below);
}

// the running base behind a chunk
CP_HD long long cp_next_base(long long base, uint64_t ballot) { return base + cp_popcount(ballot); }

// tail fill: behind the last chunk, lane `lane` writes `pad` to columns cp_tail_first(kept, lane), + CP_WAVE, ... while < L
CP_HD long long cp_tail_first(long long kept, int lane) { return kept + lane; }
