// What the kernels of a device-stepped beam search step share (beam_step.hip, beam_ctc.hip, beam_lm.hip): the log-softmax statistics of one row,
// the monotone key of an fp32 score, and the top-K selection by radix select on a unique 64-bit key.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"

namespace bsel {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

typedef unsigned long long u64;

// __syncthreads() with the LDS wait spelled out: at a loop header hipcc has dropped it
__device__ __forceinline__ void sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

// monotone 32-bit image of a score (larger = better; -0 counts as +0) and its inverse
__device__ __forceinline__ uint32_t fkey(float s) {
  if (s == 0.f) s = 0.f;
  const uint32_t u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unfkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// Row maximum of x / temperature and the logarithm of the fp64 sum of expf(x / temperature - mx), by ONE wave (every lane gets both);
// x in fp32 or bf16 (the LM's logits of beam_lm.hip)
template <typename T>
__device__ __forceinline__ void row_stats(const T* __restrict__ x, int V, float temperature, int lane, float& mx_out, float& lse_out) {
  float mx = -INFINITY;
  for (int c = lane; c < V; c += 64) mx = fmaxf(mx, Elem<T>::to_f(x[c]) / temperature);
  mx = wave_max(mx);
  double sum = 0.0;
  for (int c = lane; c < V; c += 64) sum += (double)expf(Elem<T>::to_f(x[c]) / temperature - mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  mx_out = mx;
  lse_out = (float)log(sum);
}

// The K largest of the nb * V keys key(b, c) (b < nb, c < V; unique, so the order is total), sorted descending into s_sorted[0 .. K).
// A workgroup of THREADS threads, every thread calls it; returns min(K, nb * V).  MSB-first radix select (8 bits a pass, one LDS
// histogram bin per thread, stops as soon as the bucket that holds the K-th key is taken whole), one gather pass, a rank sort.  The
// key is recomputed in every pass (V is general, a row need not fit in LDS).
template <int MAXK, typename KeyFn>
__device__ __forceinline__ int select_top(KeyFn key, int nb, int V, int K, u64* s_sorted) {
  __shared__ unsigned s_hist[THREADS], s_wtot[WAVES];
  __shared__ u64 s_sel[MAXK];
  __shared__ u64 s_prefix;
  __shared__ unsigned s_need, s_nsel;
  __shared__ int s_stop;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int iters = (V + THREADS - 1) / THREADS;
  u64 prefix = 0;
  unsigned need = (unsigned)K;
  int fshift = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    s_hist[tid] = 0;
    sync();
    for (int b = 0; b < nb; ++b)
      for (int it = 0; it < iters; ++it) {       // (the same trip count in every lane: the wave-wide ballots below see all of them)
        const int c = it * THREADS + tid;
        const bool valid = c < V;
        const u64 k = valid ? key(b, c) : 0;
        const bool in = valid && (shift == 56 || (k >> (shift + 8)) == prefix);
        const unsigned d = (unsigned)(k >> shift) & 255u;
        const u64 m = __ballot(in);
        if (m != 0) {
          // whole waves of equal digits (rows of -inf) add once instead of 64 times to one LDS word
          const int first = __ffsll((long long)m) - 1;
          const unsigned d0 = (unsigned)__shfl((int)d, first, 64);
          const u64 same = __ballot(in && d == d0);
          if (same == m) {
            if (lane == first) atomicAdd(&s_hist[d0], (unsigned)__popcll(m));
          } else if (in) {
            atomicAdd(&s_hist[d], 1u);
          }
        }
      }
    sync();
    // keys above digit tid inside the current bucket: suffix sum over the 256 bins
    const unsigned cnt = s_hist[tid];
    unsigned acc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = (unsigned)__shfl_down((int)acc, o, 64);
      if (lane + o < 64) acc += v;
    }
    if (lane == 0) s_wtot[wave] = acc;
    sync();
    unsigned above = acc - cnt;
    for (int w = wave + 1; w < WAVES; ++w) above += s_wtot[w];
    if (above < need && need <= above + cnt) {   // exactly one bin holds the need-th key from the top
      s_prefix = (prefix << 8) | (u64)tid;
      s_need = need - above;
      s_stop = cnt == need - above;              // the bucket is taken whole: the lower bits decide nothing
    }
    sync();
    prefix = s_prefix;
    need = s_need;
    fshift = shift;
    if (s_stop) break;
  }
  if (tid == 0) s_nsel = 0;
  sync();
  for (int b = 0; b < nb; ++b)
    for (int c = tid; c < V; c += THREADS) {
      const u64 k = key(b, c);
      if ((k >> fshift) >= prefix) {
        const unsigned p = atomicAdd(&s_nsel, 1u);
        if (p < (unsigned)K) s_sel[p] = k;
      }
    }
  sync();
  const int nsel = (int)min(s_nsel, (unsigned)K);
  for (int i = tid; i < nsel; i += THREADS) {
    const u64 mine = s_sel[i];
    int rank = 0;
    for (int j = 0; j < nsel; ++j) rank += s_sel[j] > mine;
    s_sorted[rank] = mine;
  }
  sync();
  return nsel;
}

}  // namespace bsel
