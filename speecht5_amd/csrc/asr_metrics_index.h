// Index arithmetic of csrc/asr_metrics.hip (greedy CTC decoding, word splitting, edit distance), as inline functions that compile
// for the device AND for the host: tests/test_asr_metrics_cpu.py builds this header with the host compiler and sweeps every offset
// against the size of the buffer it indexes before a kernel is launched.  Nothing here reads memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AM_HD __host__ __device__ __forceinline__
#else
#define AM_HD inline
#endif

constexpr int AM_ED_MAX_SHORT = 4095;   // longest "shorter sequence" the edit distance takes: 3 x 4096 ints = 48 KiB of LDS
constexpr int AM_THREADS = 256;         // threads per workgroup of every kernel of the file (= the chunk of a block prefix sum)

AM_HD int am_clamp(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// ---- greedy decoding ----
// lprobs [T, B, V]: 64-bit, T * B * V may pass 2^31
AM_HD long long am_lprobs_off(int t, int b, int v, int B, int V) { return ((long long)t * B + b) * V + v; }
// best / pred [B, T]
AM_HD long long am_row_off(int b, int i, int L) { return (long long)b * L + i; }
AM_HD int am_chunks(int n) { return (n + AM_THREADS - 1) / AM_THREADS; }
// torch's CPU argmax: does candidate (xa, ia) replace (xb, ib)?  A NaN beats every number, the lowest index wins among equals
// (among NaNs too).  ib = INT32_MAX with xb = -inf is "nothing yet": any real index beats it.
AM_HD bool am_argmax_wins(float xa, int ia, float xb, int ib) {
  const bool an = xa != xa, bn = xb != xb;
  if (an || bn) return (an && bn) ? ia < ib : an;
  if (xa != xb) return xa > xb;
  return ia < ib;
}

// ---- tokens -> bytes -> words ----
// bytes of a sentence: at most max_symbol_bytes per token
AM_HD long long am_cap(int L, int max_symbol_bytes) { return (long long)L * max_symbol_bytes; }
// words in `cap` bytes: a word is at least one byte and two words are at least one 0x20 apart
AM_HD int am_word_cap(int cap) { return (cap + 1) / 2; }

// ---- edit distance on anti-diagonals ----
// D[i][j], i in [0, s] along the SHORTER sequence, j in [0, l] along the longer one (s <= l).  Cell (i, j) lies on diagonal
// k = i + j in [0, s + l]; on diagonal k, i runs over [am_ed_lo(k, l), am_ed_hi(k, s)].  Diagonal k lives in buffer k % 3 of ONE
// array of 3 * stride ints, stride >= s + 1, at (k % 3) * stride + i.  Cell (i, j) reads (i - 1, j) and (i, j - 1) from diagonal
// k - 1 at i - 1 and i, and (i - 1, j - 1) from diagonal k - 2 at i - 1; D[s][l] ends up on diagonal s + l at index s.
AM_HD int am_ed_stride(int max_short) { return max_short + 1; }
AM_HD int am_ed_lo(int k, int l) { return k > l ? k - l : 0; }
AM_HD int am_ed_hi(int k, int s) { return k < s ? k : s; }
AM_HD int am_ed_off(int k, int i, int stride) { return (k % 3) * stride + i; }
AM_HD long long am_ed_lds_bytes(int max_short) { return 3LL * am_ed_stride(max_short) * (long long)sizeof(int32_t); }
