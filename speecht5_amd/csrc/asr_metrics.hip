// Validation UER / WER of the ASR criterion (SpeechT5/speecht5/criterions/speech_to_text_loss.py:232-297), counted on the device:
//   greedy CTC decoding of the posterior (argmax per frame, unique_consecutive, blanks dropped),
//   token rows -> the sentence's bytes through a per-symbol byte table -> words (maximal runs of bytes other than 0x20),
//   word ids (equal bytes <=> equal id between a predicted and a target word), and
//   the unit-cost Levenshtein distance of two int32 rows, once on units and once on word ids.
// Bounds discipline: every length read from device memory is clamped to its row before it bounds a loop, a token value is
// compared or range-checked and only then used as a table index, every store is guarded by the size of its buffer, and all the
// index arithmetic lives in asr_metrics_index.h, which a host test sweeps.  Plain C++: no inline assembly, no atomics.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "asr_metrics_index.h"
#include "../../include/speecht5_hip.h"

namespace {

constexpr int AM_WAVES = AM_THREADS / 64;

// Exclusive prefix sum of v over the block's AM_THREADS threads, in thread order; total = the block's sum.  Every thread of the
// block calls it (two barriers).
__device__ __forceinline__ int block_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int i = 0; i < AM_WAVES; ++i) {
    const int x = wsum[i];
    base += i < w ? x : 0;
    tot += x;
  }
  __syncthreads();
  total = tot;
  return base + inc - v;
}

// ---- greedy decoding: one wave per frame ----
__global__ __launch_bounds__(AM_THREADS) void greedy_argmax_kernel(const float* __restrict__ lp, const int64_t* __restrict__ in_len, int T,
                                                                   int B, int V, int* __restrict__ best) {
  const int lane = threadIdx.x & 63;
  const long long f = (long long)blockIdx.x * AM_WAVES + (threadIdx.x >> 6);
  if (f >= (long long)B * T) return;
  const int b = (int)(f / T), t = (int)(f % T);
  if (t >= am_clamp(in_len[b], 0, T)) return;
  float bv = -INFINITY;
  int bi = INT_MAX;
  for (int v = lane; v < V; v += 64) {
    const float x = lp[am_lprobs_off(t, b, v, B, V)];
    if (am_argmax_wins(x, v, bv, bi)) { bv = x; bi = v; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (am_argmax_wins(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) best[am_row_off(b, t, T)] = bi < V ? bi : V - 1;
}

// one workgroup per sentence: frame t is kept iff best[t] != blank and (t == 0 or best[t] != best[t - 1]); kept frames are written
// in order (block prefix sum over chunks of AM_THREADS frames, running offset), the rest of the row is -1
__global__ __launch_bounds__(AM_THREADS) void greedy_collapse_kernel(const int* __restrict__ best, const int64_t* __restrict__ in_len, int T,
                                                                     int blank, int* __restrict__ pred, int* __restrict__ pred_len) {
  __shared__ int wsum[AM_WAVES];
  const int b = blockIdx.x;
  const int Tb = am_clamp(in_len[b], 0, T);
  int run = 0;
  for (int c = 0; c < am_chunks(Tb); ++c) {
    const int t = c * AM_THREADS + threadIdx.x;
    int keep = 0, tok = 0;
    if (t < Tb) {
      tok = best[am_row_off(b, t, T)];
      keep = tok != blank && (t == 0 || tok != best[am_row_off(b, t - 1, T)]);
    }
    int tot;
    const int pos = run + block_scan(keep, wsum, tot);
    if (keep && pos < T) pred[am_row_off(b, pos, T)] = tok;
    run += tot;
  }
  run = am_clamp(run, 0, T);
  for (int i = run + threadIdx.x; i < T; i += AM_THREADS) pred[am_row_off(b, i, T)] = -1;
  if (threadIdx.x == 0) pred_len[b] = run;
}

// ---- tokens -> bytes -> words: one workgroup per sentence ----
struct WordsDims {
  int L, V, tab_bytes, max_symbol_bytes, cap, wcap;
};

__global__ __launch_bounds__(AM_THREADS) void tokens_to_words_kernel(const int* __restrict__ tokens, const int* __restrict__ len,
                                                                     const int* __restrict__ tab_off, const uint8_t* __restrict__ tab,
                                                                     WordsDims d, uint8_t* bytes, int* wstart, int* wlen,
                                                                     int* __restrict__ n_words, int* __restrict__ err) {
  __shared__ int wsum[AM_WAVES];
  const int b = blockIdx.x;
  const int n = am_clamp(len[b], 0, d.L);
  uint8_t* row = bytes + (long long)b * d.cap;
  int* ws = wstart + am_row_off(b, 0, d.wcap);
  int* wl = wlen + am_row_off(b, 0, d.wcap);
  // the sentence's bytes: token i's symbol lands at the sum of the symbol lengths before it
  int run = 0;
  for (int c = 0; c < am_chunks(n); ++c) {
    const int i = c * AM_THREADS + threadIdx.x;
    int g = 0, src = 0;
    if (i < n) {
      const int tok = tokens[am_row_off(b, i, d.L)];
      if (tok >= 0 && tok < d.V) {
        src = am_clamp(tab_off[tok], 0, d.tab_bytes);
        const int room = d.tab_bytes - src;
        g = am_clamp((long long)tab_off[tok + 1] - src, 0, room < d.max_symbol_bytes ? room : d.max_symbol_bytes);
      } else {
        err[0] = 1;      // (every writer stores the same value)
      }
    }
    int tot;
    const int dst = run + block_scan(g, wsum, tot);
    for (int j = 0; j < g; ++j)
      if (dst + j < d.cap) row[dst + j] = tab[src + j];
    run += tot;          // <= n * max_symbol_bytes <= cap
  }
  const int nb = am_clamp(run, 0, d.cap);
  __syncthreads();
  // words: byte p starts one iff it is no 0x20 and follows a 0x20 or the row's start; ends one iff no 0x20 and a 0x20 or the end follows
  int ns = 0, ne = 0;
  for (int c = 0; c < am_chunks(nb); ++c) {
    const int p = c * AM_THREADS + threadIdx.x;
    int st = 0, en = 0;
    if (p < nb) {
      const bool w = row[p] != 0x20;
      st = w && (p == 0 || row[p - 1] == 0x20);
      en = w && (p == nb - 1 || row[p + 1] == 0x20);
    }
    int ts, te;
    const int is = ns + block_scan(st, wsum, ts);
    const int ie = ne + block_scan(en, wsum, te);
    if (st && is < d.wcap) ws[is] = p;
    if (en && ie < d.wcap) wl[ie] = p + 1;
    ns += ts;
    ne += te;
  }
  const int nw = am_clamp(ns < ne ? ns : ne, 0, d.wcap);   // ns == ne: every word has one start and one end
  __syncthreads();
  for (int w = threadIdx.x; w < nw; w += AM_THREADS) wl[w] -= ws[w];
  if (threadIdx.x == 0) n_words[b] = nw;
}

// ---- word ids: one workgroup per sentence ----
struct WordRows {
  const uint8_t* bytes;
  const int* start;
  const int* len;
  const int* n;
  int cap, wcap;
};

struct Word {
  const uint8_t* p;
  int len;
};

__device__ __forceinline__ Word word_at(const WordRows& r, int b, int w) {
  const int s = am_clamp(r.start[am_row_off(b, w, r.wcap)], 0, r.cap);
  const int l = am_clamp(r.len[am_row_off(b, w, r.wcap)], 0, r.cap - s);
  return Word{r.bytes + (long long)b * r.cap + s, l};
}

__device__ __forceinline__ bool same_word(const Word& x, const Word& y) {
  if (x.len != y.len) return false;
  for (int j = 0; j < x.len; ++j)
    if (x.p[j] != y.p[j]) return false;
  return true;
}

// target word j: the index of the first target word with its bytes.  predicted word i: that index of the first target word with
// its bytes, else nt + i (no target id reaches nt).
__global__ __launch_bounds__(AM_THREADS) void word_ids_kernel(WordRows P, WordRows Tg, int* __restrict__ pid, int* __restrict__ tid) {
  const int b = blockIdx.x;
  const int np = am_clamp(P.n[b], 0, P.wcap), nt = am_clamp(Tg.n[b], 0, Tg.wcap);
  for (int w = threadIdx.x; w < np + nt; w += AM_THREADS) {
    const bool is_t = w >= np;
    const int i = is_t ? w - np : w;
    const Word me = is_t ? word_at(Tg, b, i) : word_at(P, b, i);
    const int limit = is_t ? i : nt;
    int id = is_t ? i : nt + i;
    for (int j = 0; j < limit; ++j)
      if (same_word(me, word_at(Tg, b, j))) { id = j; break; }
    if (is_t) tid[am_row_off(b, i, Tg.wcap)] = id;
    else pid[am_row_off(b, i, P.wcap)] = id;
  }
}

// ---- edit distance: one workgroup per pair, anti-diagonals, three rotating diagonals in ONE LDS array ----
__global__ __launch_bounds__(AM_THREADS) void edit_distance_kernel(const int* __restrict__ a, const int* __restrict__ a_len, int La,
                                                                   const int* __restrict__ b, const int* __restrict__ b_len, int Lb, int stride,
                                                                   int* __restrict__ dist) {
  extern __shared__ int ed[];      // 3 * stride ints, addressed as am_ed_off(k, i, stride) only
  const int r = blockIdx.x;
  const int n = am_clamp(a_len[r], 0, La), m = am_clamp(b_len[r], 0, Lb);
  const bool swapped = n > m;     // the diagonals are indexed along the shorter sequence
  const int* sh = swapped ? b + am_row_off(r, 0, Lb) : a + am_row_off(r, 0, La);
  const int* lg = swapped ? a + am_row_off(r, 0, La) : b + am_row_off(r, 0, Lb);
  const int s = swapped ? m : n, l = swapped ? n : m;
  if (am_ed_stride(s) > stride) {   // (the entry point sizes stride by min(La, Lb): not reached)
    if (threadIdx.x == 0) dist[r] = -1;
    return;
  }
  for (int k = 0; k <= s + l; ++k) {
    const int hi = am_ed_hi(k, s);
    for (int i = am_ed_lo(k, l) + threadIdx.x; i <= hi; i += AM_THREADS) {
      const int j = k - i;
      int d;
      if (i == 0) d = j;
      else if (j == 0) d = i;
      else {
        const int up = ed[am_ed_off(k - 1, i - 1, stride)];     // D[i - 1][j]
        const int left = ed[am_ed_off(k - 1, i, stride)];       // D[i][j - 1]
        const int diag = ed[am_ed_off(k - 2, i - 1, stride)];   // D[i - 1][j - 1]
        const int edit = (up < left ? up : left) + 1;
        const int sub = diag + (sh[i - 1] != lg[j - 1] ? 1 : 0);
        d = edit < sub ? edit : sub;
      }
      ed[am_ed_off(k, i, stride)] = d;
    }
    __syncthreads();   // diagonal k is complete; buffer (k + 1) % 3 held diagonal k - 2, last read while k was written
  }
  if (threadIdx.x == 0) dist[r] = ed[am_ed_off(s + l, s, stride)];
}

}  // namespace

extern "C" int st5_ctc_greedy_rows(const float* lprobs, const int64_t* input_lengths, int32_t T, int32_t B, int32_t V, int32_t blank,
                                   int32_t* best_ws, int32_t* pred, int32_t* pred_len, void* stream) {
  if (T < 0 || B < 0 || V < 1) return ST5_ERR_ARG;
  if (B == 0) return ST5_OK;
  if (!input_lengths || !pred_len || (T > 0 && (!lprobs || !best_ws || !pred))) return ST5_ERR_ARG;
  const long long blocks = ((long long)B * T + AM_WAVES - 1) / AM_WAVES;
  if (blocks > INT_MAX) return ST5_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (blocks > 0) {
    hipLaunchKernelGGL(greedy_argmax_kernel, dim3((unsigned)blocks), dim3(AM_THREADS), 0, st, lprobs, input_lengths, T, B, V, best_ws);
    HIP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(greedy_collapse_kernel, dim3(B), dim3(AM_THREADS), 0, st, best_ws, input_lengths, T, blank, pred, pred_len);
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}

extern "C" int st5_tokens_to_words(const int32_t* tokens, const int32_t* len, int32_t B, int32_t L, const int32_t* table_offsets,
                                   const uint8_t* table_bytes, int32_t V, int32_t table_nbytes, int32_t max_symbol_bytes, int32_t cap,
                                   int32_t word_cap, uint8_t* bytes, int32_t* word_start, int32_t* word_len, int32_t* n_words,
                                   int32_t* err_flag, void* stream) {
  if (B < 0 || L < 0 || V < 0 || table_nbytes < 0 || max_symbol_bytes < 0 || cap < 0 || word_cap < 0) return ST5_ERR_ARG;
  if (am_cap(L, max_symbol_bytes) != (long long)cap || word_cap != am_word_cap(cap)) return ST5_ERR_ARG;
  if (B == 0) return ST5_OK;
  if (!len || !n_words || !err_flag || !table_offsets) return ST5_ERR_ARG;
  if (L > 0 && !tokens) return ST5_ERR_ARG;
  if (cap > 0 && (!bytes || !word_start || !word_len || !table_bytes)) return ST5_ERR_ARG;
  WordsDims d{L, V, table_nbytes, max_symbol_bytes, cap, word_cap};
  hipLaunchKernelGGL(tokens_to_words_kernel, dim3(B), dim3(AM_THREADS), 0, static_cast<hipStream_t>(stream), tokens, len, table_offsets,
                     table_bytes, d, bytes, word_start, word_len, n_words, err_flag);
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}

extern "C" int st5_word_ids(const uint8_t* p_bytes, const int32_t* p_start, const int32_t* p_len, const int32_t* p_n, int32_t p_cap,
                            int32_t p_word_cap, const uint8_t* t_bytes, const int32_t* t_start, const int32_t* t_len, const int32_t* t_n,
                            int32_t t_cap, int32_t t_word_cap, int32_t B, int32_t* p_ids, int32_t* t_ids, void* stream) {
  if (B < 0 || p_cap < 0 || t_cap < 0 || p_word_cap != am_word_cap(p_cap) || t_word_cap != am_word_cap(t_cap)) return ST5_ERR_ARG;
  if (B == 0) return ST5_OK;
  if (!p_n || !t_n) return ST5_ERR_ARG;
  if (p_cap > 0 && (!p_bytes || !p_start || !p_len || !p_ids)) return ST5_ERR_ARG;
  if (t_cap > 0 && (!t_bytes || !t_start || !t_len || !t_ids)) return ST5_ERR_ARG;
  WordRows P{p_bytes, p_start, p_len, p_n, p_cap, p_word_cap};
  WordRows Tg{t_bytes, t_start, t_len, t_n, t_cap, t_word_cap};
  hipLaunchKernelGGL(word_ids_kernel, dim3(B), dim3(AM_THREADS), 0, static_cast<hipStream_t>(stream), P, Tg, p_ids, t_ids);
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}

extern "C" int st5_edit_distance_rows(const int32_t* a, const int32_t* a_len, int32_t La, const int32_t* b, const int32_t* b_len, int32_t Lb,
                                      int32_t B, int32_t* dist, void* stream) {
  if (B < 0 || La < 0 || Lb < 0) return ST5_ERR_ARG;
  const int max_short = La < Lb ? La : Lb;
  if (max_short > AM_ED_MAX_SHORT) return ST5_ERR_ARG;
  if (B == 0) return ST5_OK;
  if (!a_len || !b_len || !dist || (La > 0 && !a) || (Lb > 0 && !b)) return ST5_ERR_ARG;
  const int stride = am_ed_stride(max_short);
  hipLaunchKernelGGL(edit_distance_kernel, dim3(B), dim3(AM_THREADS), (size_t)am_ed_lds_bytes(max_short), static_cast<hipStream_t>(stream), a,
                     a_len, La, b, b_len, Lb, stride, dist);
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}
