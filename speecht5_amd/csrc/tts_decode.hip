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

// offset of this step's record column when the step index lives on the device: clamp(step[at], 0, cap - 1) * p_col (0 without a
// counter); at = 0 for the launch's one counter, b * step_ld = b for one position per row (uniform in a workgroup: a scalar load)
__device__ __forceinline__ int64_t xa_step_off(const int32_t* step, int at, int cap, int64_t p_col) {
  if (!step) return 0;
  const int s = step[at];
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
    int64_t p_head, float* __restrict__ ws, const int32_t* __restrict__ step, int step_cap, int64_t p_col, int step_ld) {
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
  float* pb = probs ? probs + (int64_t)b * p_row + (int64_t)h * p_head + xa_step_off(step, b * step_ld, step_cap, p_col) : nullptr;

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
                                                                          int step_cap, int64_t p_col, int step_ld) {
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
    const int64_t col_off = xa_step_off(step, b * step_ld, step_cap, p_col);
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
                 const int32_t* step = nullptr, int step_cap = 0, int64_t p_col = 0, int step_ld = 0) {
  const int nsplit = xa_splits(B, S);
  const int chunk = (S + nsplit - 1) / nsplit;
  const float scale = 1.0f / sqrtf((float)XA_HD);
  hipLaunchKernelGGL((decode_cross_attn_kernel<T>), dim3(nsplit, B), dim3(XA_THREADS), 0, st, static_cast<const T*>(q), q_ld,
                     static_cast<const T*>(kv), kv_ld, k_off, kpm, S, H, chunk, scale, static_cast<T*>(ctx), ctx_ld, probs, p_row, p_head,
                     nsplit > 1 ? ws : nullptr, step, step_cap, p_col, step_ld);
  if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  if (nsplit > 1) {
    hipLaunchKernelGGL((decode_cross_combine_kernel<T>), dim3(nsplit, B), dim3(XA_THREADS), 0, st, ws, S, H, chunk, static_cast<T*>(ctx),
                       ctx_ld, probs, p_row, p_head, step, step_cap, p_col, step_ld);
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
                                                              const int32_t* __restrict__ step, T* __restrict__ y, int64_t y_ld, int C,
                                                              int step_ld) {   // step_ld: 0 one counter, 1 one position per row
  const int b = blockIdx.x;
  int s = step[b * step_ld];
  s = s < 0 ? 0 : (s >= table_rows ? table_rows - 1 : s);
  const float a = alpha[0];
  const float* trow = table + (int64_t)s * C;
  for (int c = threadIdx.x; c < C; c += 256)
    y[(int64_t)b * y_ld + c] = Elem<T>::from_f(fmaf(a, trow[c], Elem<T>::to_f(x[(int64_t)b * x_ld + c])));
}

namespace {
int pe_add_entry(const void* x, int64_t x_ld, const float* table, int32_t table_rows, const float* alpha, const int32_t* step, int step_ld,
                 void* y, int64_t y_ld, int32_t B, int32_t C, int dtype, void* stream) {
  if (!x || !table || !alpha || !step || !y) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (B <= 0 || B > 65535 || C <= 0 || table_rows <= 0 || x_ld < C || y_ld < C) return ST5_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == ST5_F32)
    hipLaunchKernelGGL(tts_pe_add_step_kernel<float>, dim3(B), dim3(256), 0, st, static_cast<const float*>(x), x_ld, table, table_rows, alpha,
                       step, static_cast<float*>(y), y_ld, C, step_ld);
  else
    hipLaunchKernelGGL(tts_pe_add_step_kernel<bf16_t>, dim3(B), dim3(256), 0, st, static_cast<const bf16_t*>(x), x_ld, table, table_rows,
                       alpha, step, static_cast<bf16_t*>(y), y_ld, C, step_ld);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}
}  // namespace

extern "C" int st5_tts_pe_add_step(const void* x, int64_t x_ld, const float* table, int32_t table_rows, const float* alpha,
                                   const int32_t* step, void* y, int64_t y_ld, int32_t B, int32_t C, int dtype, void* stream) {
  return pe_add_entry(x, x_ld, table, table_rows, alpha, step, 0, y, y_ld, B, C, dtype, stream);
}

// ---- the per-row forms of a synthesis stream (speecht5_amd/tts_stream.py): pos int32 [rows] = steps completed by the current
// occupant of each row.  The cross-attention and the positional add are the kernels above with the position looked up per row. ----
extern "C" int st5_tts_pe_add_rows(const void* x, int64_t x_ld, const float* table, int32_t table_rows, const float* alpha,
                                   const int32_t* pos, void* y, int64_t y_ld, int32_t B, int32_t C, int dtype, void* stream) {
  return pe_add_entry(x, x_ld, table, table_rows, alpha, pos, 1, y, y_ld, B, C, dtype, stream);
}

extern "C" int st5_decode_cross_attn_rows(const void* q, int64_t q_ld, const void* kv, int64_t kv_ld, int64_t k_off, const uint8_t* kpm,
                                          int32_t B, int32_t S, int32_t H, int32_t head_dim, void* ctx, int64_t ctx_ld, float* probs,
                                          int64_t p_row, int64_t p_head, int64_t p_col, const int32_t* pos, int32_t cap, float* ws,
                                          int dtype, void* stream) {
  if (!q || !kv || !ctx) return ST5_ERR_ARG;
  if (head_dim != XA_HD) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (B <= 0 || B > 65535 || S <= 0 || H <= 0 || H > XA_GROUPS) return ST5_ERR_ARG;
  const int64_t C = (int64_t)H * head_dim;
  if (q_ld < C || ctx_ld < C || k_off < 0 || kv_ld < k_off + 2 * C) return ST5_ERR_ARG;
  if (probs && (!pos || cap <= 0 || p_col < S || p_head < (int64_t)cap * p_col || p_row < (int64_t)H * p_head)) return ST5_ERR_ARG;
  if (xa_splits(B, S) > 1 && !ws) return ST5_ERR_ARG;
  const int64_t vec = dtype == ST5_F32 ? 4 : 8;
  if (!aligned16(q) || !aligned16(kv) || q_ld % vec || kv_ld % vec || k_off % vec || (ws && !aligned16(ws))) return ST5_ERR_ALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == ST5_F32)
    return launch_cross<float>(q, q_ld, kv, kv_ld, k_off, kpm, B, S, H, ctx, ctx_ld, probs, p_row, p_head, ws, st, pos, cap, p_col, 1);
  return launch_cross<bf16_t>(q, q_ld, kv, kv_ld, k_off, kpm, B, S, H, ctx, ctx_ld, probs, p_row, p_head, ws, st, pos, cap, p_col, 1);
}

namespace {

// The step tail with one position per row.  One workgroup; thread b % TAIL_THREADS owns row b's state (pos, done, steps), so no cell
// is written by two threads; the frame copies read the rows' write positions from LDS behind the barrier (0 = the row writes nothing).
template <typename T>
__global__ void __launch_bounds__(TAIL_THREADS) tts_step_tail_rows_kernel(
    const float* __restrict__ y, int64_t y_ld, int B, int r, int odim, const int32_t* __restrict__ minlen,
    const int32_t* __restrict__ maxlen, int32_t* __restrict__ done, int32_t* __restrict__ steps, int32_t* __restrict__ pos, int cap,
    float threshold, float* __restrict__ mel, int64_t mel_ld, float* __restrict__ prob, int64_t prob_ld, T* __restrict__ next,
    int64_t next_ld, int32_t* __restrict__ active, int32_t* __restrict__ tick, const unsigned long long* __restrict__ seed_table,
    int table_rows, unsigned long long* __restrict__ seed_slots, int n_seeds) {
  __shared__ int32_t widx[TAIL_MAX_ROWS];      // the step (1-based) a live row writes at, 0 otherwise
  __shared__ int part[TAIL_THREADS / 64];
  const int tid = threadIdx.x;
  const int F = r * odim;
  int running = 0;
  for (int b = tid; b < B; b += TAIL_THREADS) {
    const int p = pos[b];
    const bool was = done[b] == 0 && p >= 0 && p < cap;     // (the range check in front of every address built from p)
    const int idx = p + 1;
    widx[b] = was ? idx : 0;
    if (!was) continue;
    bool hit = false;
    for (int k = 0; k < r; ++k) {
      const float pr = 1.f / (1.f + expf(-y[(int64_t)b * y_ld + F + k]));
      prob[(int64_t)b * prob_ld + (int64_t)(idx - 1) * r + k] = pr;
      hit |= pr >= threshold;
    }
    pos[b] = idx;
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
  int t1 = 0;
  if (tick) {                                  // (read by every thread in front of the barrier, written by one behind it)
    t1 = *tick + 1;
    if (t1 < 0 || t1 >= table_rows) t1 = 0;    // the tick counts modulo the seed table's rows
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < TAIL_THREADS / 64; ++w) n += part[w];
    *active = n;
    if (tick) *tick = t1;
  }
  if (tick && seed_table && tid < n_seeds) seed_slots[tid] = seed_table[(int64_t)t1 * n_seeds + tid];
  for (int64_t i = tid; i < (int64_t)B * F; i += TAIL_THREADS) {
    const int b = (int)(i / F), e = (int)(i % F);
    const int idx = widx[b];
    if (idx) mel[(int64_t)b * mel_ld + (int64_t)(idx - 1) * F + e] = y[(int64_t)b * y_ld + e];
  }
  for (int64_t i = tid; i < (int64_t)B * odim; i += TAIL_THREADS) {
    const int b = (int)(i / odim), e = (int)(i % odim);
    if (widx[b]) next[(int64_t)b * next_ld + e] = Elem<T>::from_f(y[(int64_t)b * y_ld + (r - 1) * odim + e]);
  }
}

// grid (n_admit): workgroup i hands row desc[i][0] to a new utterance.  A row index outside [0, rows) admits nothing.
template <typename T>
__global__ void __launch_bounds__(256) tts_rows_admit_kernel(const int32_t* __restrict__ desc, int rows, int32_t* __restrict__ pos,
                                                             int32_t* __restrict__ done, int32_t* __restrict__ steps,
                                                             int32_t* __restrict__ minlen, int32_t* __restrict__ maxlen,
                                                             T* __restrict__ next, int64_t next_ld, int odim, uint8_t* __restrict__ kpm, int S,
                                                             const T* __restrict__ spk_src, int64_t spk_src_ld, T* __restrict__ spk_dst,
                                                             int64_t spk_dst_ld, int D) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int b = desc[4 * i];
  if (b < 0 || b >= rows) return;
  int T_b = desc[4 * i + 1];
  T_b = T_b < 0 ? 0 : (T_b > S ? S : T_b);
  if (tid == 0) {
    pos[b] = 0;
    done[b] = 0;
    steps[b] = 0;
    minlen[b] = desc[4 * i + 2];
    maxlen[b] = desc[4 * i + 3];
  }
  for (int e = tid; e < odim; e += 256) next[(int64_t)b * next_ld + e] = Elem<T>::from_f(0.f);
  for (int j = tid; j < S; j += 256) kpm[(int64_t)b * S + j] = j >= T_b;
  if (spk_src)
    for (int d = tid; d < D; d += 256) spk_dst[(int64_t)b * spk_dst_ld + d] = spk_src[(int64_t)i * spk_src_ld + d];
}

}  // namespace

extern "C" int st5_tts_step_tail_rows(const float* y, int64_t y_ld, int32_t B, int32_t r, int32_t odim, const int32_t* minlen,
                                      const int32_t* maxlen, int32_t* done, int32_t* steps, int32_t* pos, int32_t cap, float threshold,
                                      float* mel, float* probs, void* next, int64_t next_ld, int32_t* active, int32_t* tick,
                                      const uint64_t* seed_table, int32_t table_rows, uint64_t* seed_slots, int32_t n_seeds, int dtype,
                                      void* stream) {
  if (!y || !minlen || !maxlen || !done || !steps || !mel || !probs || !next || !active || !pos) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (B <= 0 || B > TAIL_MAX_ROWS || r <= 0 || odim <= 0 || cap < 1) return ST5_ERR_ARG;
  if (y_ld < (int64_t)r * odim + r || next_ld < odim) return ST5_ERR_ARG;
  if (n_seeds < 0 || n_seeds > TAIL_THREADS || (n_seeds > 0 && (!seed_table || !seed_slots || !tick || table_rows < 1))) return ST5_ERR_ARG;
  const int64_t mel_ld = (int64_t)cap * r * odim, prob_ld = (int64_t)cap * r;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned long long* tab = reinterpret_cast<const unsigned long long*>(n_seeds ? seed_table : nullptr);
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(n_seeds ? seed_slots : nullptr);
  if (!tick || table_rows < 1) table_rows = 1;
  if (dtype == ST5_F32)
    hipLaunchKernelGGL(tts_step_tail_rows_kernel<float>, dim3(1), dim3(TAIL_THREADS), 0, st, y, y_ld, B, r, odim, minlen, maxlen, done,
                       steps, pos, cap, threshold, mel, mel_ld, probs, prob_ld, static_cast<float*>(next), next_ld, active, tick, tab,
                       table_rows, slots, n_seeds);
  else
    hipLaunchKernelGGL(tts_step_tail_rows_kernel<bf16_t>, dim3(1), dim3(TAIL_THREADS), 0, st, y, y_ld, B, r, odim, minlen, maxlen, done,
                       steps, pos, cap, threshold, mel, mel_ld, probs, prob_ld, static_cast<bf16_t*>(next), next_ld, active, tick, tab,
                       table_rows, slots, n_seeds);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_tts_rows_admit(const int32_t* desc, int32_t n_admit, int32_t rows, int32_t* pos, int32_t* done, int32_t* steps,
                                  int32_t* minlen, int32_t* maxlen, void* next, int64_t next_ld, int32_t odim, uint8_t* kpm, int32_t S,
                                  const void* spk_src, int64_t spk_src_ld, void* spk_dst, int64_t spk_dst_ld, int32_t D, int dtype,
                                  void* stream) {
  if (n_admit == 0) return ST5_OK;
  if (!desc || !pos || !done || !steps || !minlen || !maxlen || !next || !kpm) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (n_admit < 0 || n_admit > rows || rows <= 0 || rows > 65535 || odim <= 0 || next_ld < odim || S <= 0) return ST5_ERR_ARG;
  if (spk_src && (!spk_dst || D <= 0 || spk_src_ld < D || spk_dst_ld < D)) return ST5_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == ST5_F32)
    hipLaunchKernelGGL(tts_rows_admit_kernel<float>, dim3(n_admit), dim3(256), 0, st, desc, rows, pos, done, steps, minlen, maxlen,
                       static_cast<float*>(next), next_ld, odim, kpm, S, static_cast<const float*>(spk_src), spk_src_ld,
                       static_cast<float*>(spk_dst), spk_dst_ld, D);
  else
    hipLaunchKernelGGL(tts_rows_admit_kernel<bf16_t>, dim3(n_admit), dim3(256), 0, st, desc, rows, pos, done, steps, minlen, maxlen,
                       static_cast<bf16_t*>(next), next_ld, odim, kpm, S, static_cast<const bf16_t*>(spk_src), spk_src_ld,
                       static_cast<bf16_t*>(spk_dst), spk_dst_ld, D);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}
