// Batched speech synthesis (T5TransformerModel.generate_speech_batch): the two kernels of a decode step that the single-utterance
// loop (SpeechT5/speecht5/models/speecht5.py:1188-1249) runs as many small launches and one host read.
//
// st5_decode_cross_attn: the cross-attention of multihead_attention.py:340-389 with ONE query per row b:
//   ctx[b, h*64:(h+1)*64] = softmax_j(q_h . K_h[b, j]^T * 64^-0.5) . V_h[b, j] over the S encoder positions of row b, keys whose
//   padding byte is set excluded (probability exactly 0).  Scores, softmax and accumulation in fp32.  A workgroup takes one row and
//   a range of keys, ALL heads: groups of 4 lanes own one (key, head) pair and hold 16 of its 64 elements (bf16: one 16-byte load of
//   K and one of V per 8 elements).  Once S > XA_SPLIT_MIN the key range is split over several workgroups and a second kernel
//   combines the partial (max, sum, acc) states -- the hand-off between workgroups is the kernel boundary, as in lm_decode.hip.
//   With `probs` set the raw scores go to the caller's record first and are normalised in place once the row's max / sum are
//   known: by the lane that wrote them (one workgroup) or by the combine kernel (split).  The context never reads the record, so
//   ctx is the same bits with and without it.
// st5_tts_step_tail: the stop rule of every row (speecht5.py:1240-1246), the frame / probability record, the next decoder input and
//   the count of rows still running, in one workgroup (integer LDS reduction, no atomics).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "../../include/speecht5_hip.h"

namespace {

constexpr int XA_THREADS = 256;
constexpr int XA_GROUPS = XA_THREADS / 4;   // 4 lanes per (key, head)
constexpr int XA_HD = 64;
constexpr int XA_EPL = XA_HD / 4;           // 16 elements per lane
constexpr int XA_SPLIT_MIN = 64;            // up to this many keys one workgroup per row covers them all
constexpr int XA_SPLIT_CHUNK = 16;          // fewest keys per workgroup once split
constexpr int XA_SPLIT_MAX = 128;
constexpr int XA_TARGET_BLOCKS = 1024;      // 4 workgroups per CU
constexpr int TAIL_THREADS = 256;
constexpr int TAIL_MAX_ROWS = 4096;

__host__ __device__ inline int xa_splits(int B, int S) {
  if (S <= XA_SPLIT_MIN) return 1;
  int want = (XA_TARGET_BLOCKS + B - 1) / B;
  const int most = (S + XA_SPLIT_CHUNK - 1) / XA_SPLIT_CHUNK;
  if (want > most) want = most;
  if (want > XA_SPLIT_MAX) want = XA_SPLIT_MAX;
  return want < 2 ? 2 : want;
}

// offset of this step's record column when the step index lives on the device: clamp(*step, 0, cap - 1) * p_col (0 without a counter)
__device__ __forceinline__ int64_t xa_step_off(const int32_t* step, int cap, int64_t p_col) {
  if (!step) return 0;
  const int s = *step;
  return (int64_t)(s < 0 ? 0 : (s >= cap ? cap - 1 : s)) * p_col;
}

// 16 consecutive elements as floats: fp32 four 16-byte loads, bf16 two
template <typename T>
__device__ __forceinline__ void load16f(const T* p, float* v) {
  float a[8], b[8];
  load8f<T>(p, a);
  load8f<T>(p + 8, b);
#pragma unroll
  for (int e = 0; e < 8; ++e) { v[e] = a[e]; v[8 + e] = b[e]; }
}

// grid (nsplit, B).  ws == nullptr (nsplit 1): ctx is written and the record normalised here.  Otherwise ws holds per (row, split):
// H maxima, H sums, then the C unnormalised accumulators; the record holds raw scores until the combine kernel.
template <typename T>
__global__ void __launch_bounds__(XA_THREADS) decode_cross_attn_kernel(
    const T* __restrict__ q, int64_t q_ld, const T* __restrict__ kv, int64_t kv_ld, int64_t k_off, const uint8_t* __restrict__ kpm,
    int S, int H, int chunk, float scale, T* __restrict__ ctx, int64_t ctx_ld, float* __restrict__ probs, int64_t p_row,
    int64_t p_head, float* __restrict__ ws, const int32_t* __restrict__ step, int step_cap, int64_t p_col) {
  const int C = H * XA_HD;
  const int b = blockIdx.y, split = blockIdx.x, nsplit = gridDim.x;
  const int tid = threadIdx.x, g = tid >> 2, sub = tid & 3;
  const int P = XA_GROUPS / H;                // keys in flight per pass
  const int h = g % H, ps = g / H;
  const bool active = ps < P;
  const int j0 = split * chunk;
  const int j1 = min(S, j0 + chunk);
  const int col = h * XA_HD + sub * XA_EPL;
  const T* kvb = kv + (int64_t)b * S * kv_ld + k_off + col;
  const uint8_t* mb = kpm ? kpm + (int64_t)b * S : nullptr;
  float* pb = probs ? probs + (int64_t)b * p_row + (int64_t)h * p_head + xa_step_off(step, step_cap, p_col) : nullptr;

  float qf[XA_EPL], acc[XA_EPL];
  float m = -INFINITY, l = 0.f;
#pragma unroll
  for (int e = 0; e < XA_EPL; ++e) acc[e] = 0.f;
  if (active) {
    load16f<T>(q + (int64_t)b * q_ld + col, qf);
#pragma unroll
    for (int e = 0; e < XA_EPL; ++e) qf[e] *= scale;
  }
  for (int jb = j0; jb < j1; jb += P) {
    const int j = jb + ps;
    const bool on = active && j < j1;
    const bool valid = on && !(mb && mb[j]);
    float vf[XA_EPL];
    float s = -INFINITY;
    if (valid) {
      float kf[XA_EPL];
      const T* row = kvb + (int64_t)j * kv_ld;
      load16f<T>(row, kf);
      load16f<T>(row + C, vf);
      s = 0.f;
#pragma unroll
      for (int e = 0; e < XA_EPL; ++e) s = fmaf(qf[e], kf[e], s);
    }
    // (the 4 lanes of a group share j, so they agree on `valid`; every lane of the wave takes part in the shuffles)
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (valid) {
      const float mn = fmaxf(m, s);
      const float corr = expf(m - mn), p = expf(s - mn);
      l = l * corr + p;
#pragma unroll
      for (int e = 0; e < XA_EPL; ++e) acc[e] = fmaf(p, vf[e], acc[e] * corr);
      m = mn;
    }
    if (on && pb && sub == 0) pb[j] = s;      // raw score (-inf at a padded key), normalised below or by the combine kernel
  }

  // combine the P key lanes of each head through LDS
  __shared__ float s_m[XA_GROUPS], s_l[XA_GROUPS];
  __shared__ float s_acc[XA_GROUPS * XA_HD];  // P * C = (64 / H) * H * 64 <= 64 * 64
  __shared__ float s_M[XA_GROUPS], s_L[XA_GROUPS];
  if (active) {
    if (sub == 0) { s_m[ps * H + h] = m; s_l[ps * H + h] = l; }
#pragma unroll
    for (int e = 0; e < XA_EPL; ++e) s_acc[ps * C + col + e] = acc[e];
  }
  __syncthreads();
  for (int c = tid; c < C; c += XA_THREADS) {
    const int hh = c / XA_HD;
    float M = -INFINITY;
    for (int p = 0; p < P; ++p) M = fmaxf(M, s_m[p * H + hh]);
    float L = 0.f, A = 0.f;
    if (M != -INFINITY) {
      for (int p = 0; p < P; ++p) {
        const float w = expf(s_m[p * H + hh] - M);
        L = fmaf(w, s_l[p * H + hh], L);
        A = fmaf(w, s_acc[p * C + c], A);
      }
    }
    if (ws == nullptr) {
      ctx[(int64_t)b * ctx_ld + c] = Elem<T>::from_f(A / L);
      if (c % XA_HD == 0) { s_M[hh] = M; s_L[hh] = L; }
    } else {
      float* w = ws + ((int64_t)b * nsplit + split) * (2 * H + C);
      if (c % XA_HD == 0) { w[hh] = M; w[H + hh] = L; }
      w[2 * H + c] = A;
    }
  }
  if (ws == nullptr && pb) {
    __syncthreads();
    if (active && sub == 0) {
      const float M = s_M[h], L = s_L[h];
      for (int j = j0 + ps; j < j1; j += P) pb[j] = expf(pb[j] - M) / L;   // each lane re-reads only what it wrote
    }
  }
}

// grid (nsplit, B): every workgroup of row b merges the row's nsplit partial states per head, writes its share of the C context
// columns, and normalises the record entries of its own key range.
template <typename T>
__global__ void __launch_bounds__(XA_THREADS) decode_cross_combine_kernel(const float* __restrict__ ws, int S, int H, int chunk,
                                                                          T* __restrict__ ctx, int64_t ctx_ld, float* __restrict__ probs,
                                                                          int64_t p_row, int64_t p_head, const int32_t* __restrict__ step,
                                                                          int step_cap, int64_t p_col) {
  const int b = blockIdx.y, split = blockIdx.x, nsplit = gridDim.x, tid = threadIdx.x;
  const int C = H * XA_HD;
  const int64_t stride = 2 * H + C;
  const float* base = ws + (int64_t)b * nsplit * stride;
  __shared__ float s_M[XA_GROUPS], s_L[XA_GROUPS];
  for (int h = tid; h < H; h += XA_THREADS) {
    float M = -INFINITY;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, base[s * stride + h]);
    float L = 0.f;
    if (M != -INFINITY) {
      for (int s = 0; s < nsplit; ++s) {
        const float ms = base[s * stride + h];
        L = fmaf(ms == -INFINITY ? 0.f : expf(ms - M), base[s * stride + H + h], L);   // (a split without valid keys adds 0)
      }
    }
    s_M[h] = M;
    s_L[h] = L;
  }
  __syncthreads();
  for (int c = split * XA_THREADS + tid; c < C; c += nsplit * XA_THREADS) {
    const int h = c / XA_HD;
    const float M = s_M[h];
    float A = 0.f;
    if (M != -INFINITY) {
      for (int s = 0; s < nsplit; ++s) {
        const float ms = base[s * stride + h];
        A = fmaf(ms == -INFINITY ? 0.f : expf(ms - M), base[s * stride + 2 * H + c], A);
      }
    }
    ctx[(int64_t)b * ctx_ld + c] = Elem<T>::from_f(A / s_L[h]);
  }
  if (probs) {
    const int j0 = split * chunk;
    const int n = min(S, j0 + chunk) - j0;
    if (n <= 0) return;
    const int64_t col_off = xa_step_off(step, step_cap, p_col);
    for (int i = tid; i < H * n; i += XA_THREADS) {
      const int h = i / n, j = j0 + i % n;
      float* p = probs + (int64_t)b * p_row + (int64_t)h * p_head + j + col_off;
      *p = expf(*p - s_M[h]) / s_L[h];
    }
  }
}

template <typename T>
int launch_cross(const void* q, int64_t q_ld, const void* kv, int64_t kv_ld, int64_t k_off, const uint8_t* kpm, int B, int S, int H,
                 void* ctx, int64_t ctx_ld, float* probs, int64_t p_row, int64_t p_head, float* ws, hipStream_t st,
                 const int32_t* step = nullptr, int step_cap = 0, int64_t p_col = 0) {
  const int nsplit = xa_splits(B, S);
  const int chunk = (S + nsplit - 1) / nsplit;
  const float scale = 1.0f / sqrtf((float)XA_HD);
  hipLaunchKernelGGL((decode_cross_attn_kernel<T>), dim3(nsplit, B), dim3(XA_THREADS), 0, st, static_cast<const T*>(q), q_ld,
                     static_cast<const T*>(kv), kv_ld, k_off, kpm, S, H, chunk, scale, static_cast<T*>(ctx), ctx_ld, probs, p_row, p_head,
                     nsplit > 1 ? ws : nullptr, step, step_cap, p_col);
  if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  if (nsplit > 1) {
    hipLaunchKernelGGL((decode_cross_combine_kernel<T>), dim3(nsplit, B), dim3(XA_THREADS), 0, st, ws, S, H, chunk, static_cast<T*>(ctx),
                       ctx_ld, probs, p_row, p_head, step, step_cap, p_col);
    if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  }
  return ST5_OK;
}

template <typename T>
__global__ void __launch_bounds__(TAIL_THREADS) tts_step_tail_kernel(
    const float* __restrict__ y, int64_t y_ld, int B, int r, int odim, const int32_t* __restrict__ minlen,
    const int32_t* __restrict__ maxlen, int32_t* __restrict__ done, int32_t* __restrict__ steps, int idx, float threshold,
    float* __restrict__ mel, int64_t mel_ld, float* __restrict__ prob, int64_t prob_ld, T* __restrict__ next, int64_t next_ld,
    int32_t* __restrict__ active, int32_t* __restrict__ counter, int cap, const unsigned long long* __restrict__ seed_table,
    unsigned long long* __restrict__ seed_slots, int n_seeds) {
  __shared__ uint8_t live[TAIL_MAX_ROWS];
  __shared__ int part[TAIL_THREADS / 64];
  const int tid = threadIdx.x;
  if (counter) {                               // step index on the device: this is step *counter + 1; past the cap nothing is written
    idx = *counter + 1;
    if (idx < 1 || idx > cap) return;
  }
  const int F = r * odim;
  int running = 0;
  for (int b = tid; b < B; b += TAIL_THREADS) {
    const bool was = done[b] == 0;
    live[b] = was;
    if (!was) continue;
    bool hit = false;
    for (int k = 0; k < r; ++k) {
      const float p = 1.f / (1.f + expf(-y[(int64_t)b * y_ld + F + k]));
      prob[(int64_t)b * prob_ld + (int64_t)(idx - 1) * r + k] = p;
      hit |= p >= threshold;
    }
    if (idx >= minlen[b] && (hit || idx >= maxlen[b])) {
      done[b] = 1;
      steps[b] = idx;
    } else {
      ++running;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) running += __shfl_xor(running, o, 64);
  if ((tid & 63) == 0) part[tid >> 6] = running;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < TAIL_THREADS / 64; ++w) n += part[w];
    *active = n;
    if (counter) *counter = idx;               // (every thread read it in front of the barrier above)
  }
  if (counter && seed_table && tid < n_seeds && idx < cap) seed_slots[tid] = seed_table[(int64_t)idx * n_seeds + tid];
  for (int64_t i = tid; i < (int64_t)B * F; i += TAIL_THREADS) {
    const int b = (int)(i / F), e = (int)(i % F);
    if (live[b]) mel[(int64_t)b * mel_ld + (int64_t)(idx - 1) * F + e] = y[(int64_t)b * y_ld + e];
  }
  for (int64_t i = tid; i < (int64_t)B * odim; i += TAIL_THREADS) {
    const int b = (int)(i / odim), e = (int)(i % odim);
    if (live[b]) next[(int64_t)b * next_ld + e] = Elem<T>::from_f(y[(int64_t)b * y_ld + (r - 1) * odim + e]);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int64_t st5_decode_cross_attn_ws_bytes(int32_t B, int32_t S, int32_t H, int32_t head_dim) {
  if (B <= 0 || S <= 0 || H <= 0 || head_dim <= 0) return 0;
  const int nsplit = xa_splits(B, S);
  return nsplit > 1 ? (int64_t)B * nsplit * (2 * H + (int64_t)H * head_dim) * 4 : 0;
}

extern "C" int st5_decode_cross_attn(const void* q, int64_t q_ld, const void* kv, int64_t kv_ld, int64_t k_off, const uint8_t* kpm,
                                     int32_t B, int32_t S, int32_t H, int32_t head_dim, void* ctx, int64_t ctx_ld, float* probs,
                                     int64_t p_row, int64_t p_head, float* ws, int dtype, void* stream) {
  if (!q || !kv || !ctx) return ST5_ERR_ARG;
  if (head_dim != XA_HD) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (B <= 0 || B > 65535 || S <= 0 || H <= 0 || H > XA_GROUPS) return ST5_ERR_ARG;
  const int64_t C = (int64_t)H * head_dim;
  if (q_ld < C || ctx_ld < C || k_off < 0 || kv_ld < k_off + 2 * C) return ST5_ERR_ARG;
  if (probs && (p_head < S || p_row < (int64_t)H * p_head)) return ST5_ERR_ARG;
  if (xa_splits(B, S) > 1 && !ws) return ST5_ERR_ARG;
  const int64_t vec = dtype == ST5_F32 ? 4 : 8;   // 16-byte rows: every lane's loads stay aligned
  if (!aligned16(q) || !aligned16(kv) || q_ld % vec || kv_ld % vec || k_off % vec || (ws && !aligned16(ws))) return ST5_ERR_ALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == ST5_F32)
    return launch_cross<float>(q, q_ld, kv, kv_ld, k_off, kpm, B, S, H, ctx, ctx_ld, probs, p_row, p_head, ws, st);
  return launch_cross<bf16_t>(q, q_ld, kv, kv_ld, k_off, kpm, B, S, H, ctx, ctx_ld, probs, p_row, p_head, ws, st);
}

extern "C" int st5_tts_step_tail(const float* y, int64_t y_ld, int32_t B, int32_t r, int32_t odim, const int32_t* minlen,
                                 const int32_t* maxlen, int32_t* done, int32_t* steps, int32_t idx, int32_t cap, float threshold, float* mel,
                                 float* probs, void* next, int64_t next_ld, int32_t* active, int dtype, void* stream) {
  if (!y || !minlen || !maxlen || !done || !steps || !mel || !probs || !next || !active) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (B <= 0 || B > TAIL_MAX_ROWS || r <= 0 || odim <= 0 || idx < 1 || idx > cap) return ST5_ERR_ARG;
  if (y_ld < (int64_t)r * odim + r || next_ld < odim) return ST5_ERR_ARG;
  const int64_t mel_ld = (int64_t)cap * r * odim, prob_ld = (int64_t)cap * r;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == ST5_F32)
    hipLaunchKernelGGL(tts_step_tail_kernel<float>, dim3(1), dim3(TAIL_THREADS), 0, st, y, y_ld, B, r, odim, minlen, maxlen, done, steps,
                       idx, threshold, mel, mel_ld, probs, prob_ld, static_cast<float*>(next), next_ld, active, nullptr, cap, nullptr, nullptr, 0);
  else
    hipLaunchKernelGGL(tts_step_tail_kernel<bf16_t>, dim3(1), dim3(TAIL_THREADS), 0, st, y, y_ld, B, r, odim, minlen, maxlen, done, steps,
                       idx, threshold, mel, mel_ld, probs, prob_ld, static_cast<bf16_t*>(next), next_ld, active, nullptr, cap, nullptr, nullptr, 0);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

// ---- the same three with the step index in device memory (one int32 counter c = steps completed, owned by the decode state) ----
extern "C" int st5_decode_cross_attn_step(const void* q, int64_t q_ld, const void* kv, int64_t kv_ld, int64_t k_off, const uint8_t* kpm,
                                          int32_t B, int32_t S, int32_t H, int32_t head_dim, void* ctx, int64_t ctx_ld, float* probs,
                                          int64_t p_row, int64_t p_head, int64_t p_col, const int32_t* step, int32_t cap, float* ws,
                                          int dtype, void* stream) {
  if (!q || !kv || !ctx) return ST5_ERR_ARG;
  if (head_dim != XA_HD) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (B <= 0 || B > 65535 || S <= 0 || H <= 0 || H > XA_GROUPS) return ST5_ERR_ARG;
  const int64_t C = (int64_t)H * head_dim;
  if (q_ld < C || ctx_ld < C || k_off < 0 || kv_ld < k_off + 2 * C) return ST5_ERR_ARG;
  if (probs && (!step || cap <= 0 || p_col < S || p_head < (int64_t)cap * p_col || p_row < (int64_t)H * p_head)) return ST5_ERR_ARG;
  if (xa_splits(B, S) > 1 && !ws) return ST5_ERR_ARG;
  const int64_t vec = dtype == ST5_F32 ? 4 : 8;
  if (!aligned16(q) || !aligned16(kv) || q_ld % vec || kv_ld % vec || k_off % vec || (ws && !aligned16(ws))) return ST5_ERR_ALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == ST5_F32)
    return launch_cross<float>(q, q_ld, kv, kv_ld, k_off, kpm, B, S, H, ctx, ctx_ld, probs, p_row, p_head, ws, st, step, cap, p_col);
  return launch_cross<bf16_t>(q, q_ld, kv, kv_ld, k_off, kpm, B, S, H, ctx, ctx_ld, probs, p_row, p_head, ws, st, step, cap, p_col);
}

extern "C" int st5_tts_step_tail_dev(const float* y, int64_t y_ld, int32_t B, int32_t r, int32_t odim, const int32_t* minlen,
                                     const int32_t* maxlen, int32_t* done, int32_t* steps, int32_t* counter, int32_t cap, float threshold,
                                     float* mel, float* probs, void* next, int64_t next_ld, int32_t* active, const uint64_t* seed_table,
                                     uint64_t* seed_slots, int32_t n_seeds, int dtype, void* stream) {
  if (!y || !minlen || !maxlen || !done || !steps || !mel || !probs || !next || !active || !counter) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (B <= 0 || B > TAIL_MAX_ROWS || r <= 0 || odim <= 0 || cap < 1) return ST5_ERR_ARG;
  if (y_ld < (int64_t)r * odim + r || next_ld < odim) return ST5_ERR_ARG;
  if (n_seeds < 0 || n_seeds > TAIL_THREADS || (n_seeds > 0 && (!seed_table || !seed_slots))) return ST5_ERR_ARG;
  const int64_t mel_ld = (int64_t)cap * r * odim, prob_ld = (int64_t)cap * r;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned long long* tab = reinterpret_cast<const unsigned long long*>(n_seeds ? seed_table : nullptr);
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(n_seeds ? seed_slots : nullptr);
  if (dtype == ST5_F32)
    hipLaunchKernelGGL(tts_step_tail_kernel<float>, dim3(1), dim3(TAIL_THREADS), 0, st, y, y_ld, B, r, odim, minlen, maxlen, done, steps,
                       0, threshold, mel, mel_ld, probs, prob_ld, static_cast<float*>(next), next_ld, active, counter, cap, tab, slots, n_seeds);
  else
    hipLaunchKernelGGL(tts_step_tail_kernel<bf16_t>, dim3(1), dim3(TAIL_THREADS), 0, st, y, y_ld, B, r, odim, minlen, maxlen, done, steps,
                       0, threshold, mel, mel_ld, probs, prob_ld, static_cast<bf16_t*>(next), next_ld, active, counter, cap, tab, slots, n_seeds);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

// y[b, :C] = x[b, :C] + alpha[0] * table[clamp(*step, 0, table_rows - 1), :C]: the scaled positional row of the step whose index lives
// on the device (ScaledPEAdd with pos_offset = *step), written at a caller-chosen row stride (the left part of [x ; speaker] rows).
template <typename T>
__global__ void __launch_bounds__(256) tts_pe_add_step_kernel(const T* __restrict__ x, int64_t x_ld, const float* __restrict__ table,
                                                              int table_rows, const float* __restrict__ alpha,
                                                              const int32_t* __restrict__ step, T* __restrict__ y, int64_t y_ld, int C) {
  const int b = blockIdx.x;
  int s = *step;
  s = s < 0 ? 0 : (s >= table_rows ? table_rows - 1 : s);
  const float a = alpha[0];
  const float* trow = table + (int64_t)s * C;
  for (int c = threadIdx.x; c < C; c += 256)
    y[(int64_t)b * y_ld + c] = Elem<T>::from_f(fmaf(a, trow[c], Elem<T>::to_f(x[(int64_t)b * x_ld + c])));
}

extern "C" int st5_tts_pe_add_step(const void* x, int64_t x_ld, const float* table, int32_t table_rows, const float* alpha,
                                   const int32_t* step, void* y, int64_t y_ld, int32_t B, int32_t C, int dtype, void* stream) {
  if (!x || !table || !alpha || !step || !y) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (B <= 0 || B > 65535 || C <= 0 || table_rows <= 0 || x_ld < C || y_ld < C) return ST5_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == ST5_F32)
    hipLaunchKernelGGL(tts_pe_add_step_kernel<float>, dim3(B), dim3(256), 0, st, static_cast<const float*>(x), x_ld, table, table_rows, alpha,
                       step, static_cast<float*>(y), y_ld, C);
  else
    hipLaunchKernelGGL(tts_pe_add_step_kernel<bf16_t>, dim3(B), dim3(256), 0, st, static_cast<const bf16_t*>(x), x_ld, table, table_rows,
                       alpha, step, static_cast<bf16_t*>(y), y_ld, C);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}
