// Beam search over a slot cache (SequenceGenerator(decode="slots")): the cross-attention of a decode step in which all `beam`
// hypothesis rows of a sentence read ONE copy of that sentence's projected encoder keys / values.
//
// st5_beam_cross_attn: the cross-attention of multihead_attention.py:340-389 with one query per hypothesis row r:
//   ctx[r, h*64:(h+1)*64] = softmax_j(q_h[r] . K_h[s, j]^T * 64^-0.5) . V_h[s, j],  s = sent[r / beam], over the S encoder positions
//   of sentence s, keys whose padding byte is set excluded (probability exactly 0).  Scores, softmax and accumulation in fp32.
// Work division: a workgroup owns one live sentence and a range of keys, all heads (32 per workgroup) and all beam rows (16 per
//   workgroup; beams over 16 and more than 32 heads run as further workgroups along grid.z).  Groups of 8 lanes own one
//   (key, head) pair: each lane loads 8 of the 64 elements of K and of V straight into VGPRs (bf16: one 16-byte load each) and uses
//   them for EVERY row of the workgroup, so a K / V element is read from memory once per sentence and step.  The queries of the
//   workgroup's rows sit in LDS (pre-scaled, 8-element pieces XOR-swizzled by the head so that the heads of a wave hit different
//   banks); every row keeps its own online-softmax state (max, sum, 8 accumulators per lane) in registers.
// Scores are VALU dot products, not MFMA: with K on the lanes of mfma_f32_16x16x32_bf16 the probabilities come out with the key on
//   the register index, and P.V then needs V transposed (keys along k) -- an LDS round trip for an operand that is streamed once;
//   fp32 operands would need a second code path (16x16x4); the dot products keep K/V in registers and one code path for both dtypes.
//   Measured (profiles/beam_slots_*): the kernel is NOT bound by the K/V stream.  At Base, 8 sentences x beam 10,
//   S 499, bf16 it takes 47 us + 7 us combine, 12.3 MB of K|V once per sentence = 0.26 TB/s: 256 workgroups of one wave per SIMD, each
//   walking 8 passes of 2 keys through 16 register rows (6 of them idle at beam 10, 8 of the 32 lane groups idle at 12 heads) and
//   writing fp32 partials (8 MB) next to the 12 MB it reads.  32 keys per workgroup is faster at 32 sentences (83 against 109 us) and
//   slower at 8 and 1 (68 / 65 against 52 / 46 us), 64 keys slower everywhere (profiles/beam_slots_chunk_ab.txt): at 8 sentences the
//   launch is short of workgroups, not of bandwidth.  BX_CHUNK_KEYS stays at 16, the better choice at the acceptance size.
// Reduction order: the key range is split by S alone (bx_splits), the keys of a range go round the 32 / min(H, 32) key lanes of a
//   head in turn, the key lanes combine in lane order through LDS and the ranges in range order in the combine kernel.  None of it
//   depends on n_live, beam or the other rows of the launch: a row's ctx bits are a function of its query and its sentence.
//   The hand-off between workgroups is the kernel boundary (as in lm_decode.hip / tts_decode.hip); no atomics.
// With `probs` set the raw (log2-domain) scores go to the caller's record first and are normalised in place once the row's max /
//   sum are known: by the lane that wrote them (one range) or by the combine kernel (split).  ctx never reads the record.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "../../include/speecht5_hip.h"

namespace {

constexpr int BX_THREADS = 256;
constexpr int BX_LPG = 8;                        // lanes per (key, head)
constexpr int BX_GROUPS = BX_THREADS / BX_LPG;   // 32 (key, head) pairs in flight; also the heads of one workgroup
constexpr int BX_HD = 64;
constexpr int BX_EPL = BX_HD / BX_LPG;           // 8 elements per lane
constexpr int BX_MAX_ROWS = 16;                  // hypothesis rows per workgroup
constexpr int BX_SINGLE_MAX = 64;                // up to this many keys one workgroup per sentence covers them all
#ifndef BX_CHUNK_KEYS
#define BX_CHUNK_KEYS 16
#endif
constexpr int BX_CHUNK = BX_CHUNK_KEYS;          // keys per workgroup once split
constexpr int BX_SPLIT_MAX = 128;
constexpr int BX_COMB_FLOATS = 4 * BX_GROUPS + BX_GROUPS * BX_HD;   // LDS of the key-lane combine (re-uses the query image)
constexpr float BX_LOG2E = 1.4426950408889634f;

// (a function of S only: the reduction order of a row must not depend on what else is launched)
__host__ __device__ inline int bx_splits(int S) {
  if (S <= BX_SINGLE_MAX) return 1;
  const int n = (S + BX_CHUNK - 1) / BX_CHUNK;
  return n > BX_SPLIT_MAX ? BX_SPLIT_MAX : n;
}

__host__ inline int bx_rows_per_block(int H, int beam) {
  const int hc = H < BX_GROUPS ? H : BX_GROUPS;
  const int cap = hc <= 16 ? BX_MAX_ROWS : 8;    // query image rows * hc * 64 * 4 bytes <= 64 KiB
  const int want = beam < cap ? beam : cap;
  int rb = 1;
  while (rb < want) rb *= 2;
  return rb;
}

__device__ __forceinline__ float bx_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// sum over the 8 lanes of a group, the same bits in all 8 (quad xor 1, quad xor 2, mirror inside the half row)
__device__ __forceinline__ float bx_group_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));   // row_half_mirror
  return v;
}

// grid (nsplit, n_live, row groups * head chunks).  ws == nullptr (nsplit 1): ctx is written and the record normalised here.
// Otherwise ws holds per (row, split): H maxima, H sums (log2 domain), then the C unnormalised accumulators; the record holds raw
// scores until the combine kernel.  Dynamic LDS: max(RB * Hc * 64, BX_COMB_FLOATS) floats.
template <typename T, int RB>
__global__ void __launch_bounds__(BX_THREADS) beam_cross_attn_kernel(
    const T* __restrict__ q, int64_t q_ld, const T* __restrict__ kv, int64_t kv_ld, int64_t k_off, const uint8_t* __restrict__ kpm,
    const int32_t* __restrict__ sent, int n_sent, int beam, int S, int H, int chunk, float qscale, T* __restrict__ ctx, int64_t ctx_ld,
    float* __restrict__ probs, int64_t p_row, int64_t p_head, float* __restrict__ ws, int nhc) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int C = H * BX_HD;
  const int split = blockIdx.x, nsplit = gridDim.x, live = blockIdx.y;
  const int grp = blockIdx.z / nhc, hc = blockIdx.z % nhc;
  const int h0 = hc * BX_GROUPS;
  const int Hc = min(BX_GROUPS, H - h0), Cc = Hc * BX_HD;
  const int nr = min(RB, beam - grp * RB);      // rows of this workgroup (the rest of the RB register rows run on zero queries)
  const int64_t row0 = (int64_t)live * beam + (int64_t)grp * RB;
  const int tid = threadIdx.x, g = tid >> 3, sub = tid & 7;
  const int P = BX_GROUPS / Hc;                 // keys in flight per pass
  const int h = g % Hc, ps = g / Hc;
  const bool active = ps < P;
  const int j0 = split * chunk;
  const int j1 = min(S, j0 + chunk);
  const int sidx = sent[live];
  if (sidx < 0 || sidx >= n_sent) {             // a broken sentence entry shows up in the output, it is never dereferenced
    if (ws != nullptr) return;                  // (split: the combine kernel writes the NaNs)
    for (int i = tid; i < nr * Cc; i += BX_THREADS)
      ctx[(row0 + i / Cc) * ctx_ld + h0 * BX_HD + i % Cc] = Elem<T>::from_f(NAN);
    if (probs)
      for (int64_t i = tid; i < (int64_t)nr * Hc * S; i += BX_THREADS) {
        const int r = (int)(i / ((int64_t)Hc * S)), hh = (int)(i / S) % Hc, j = (int)(i % S);
        probs[(row0 + r) * p_row + (int64_t)(h0 + hh) * p_head + j] = NAN;
      }
    return;
  }

  // the queries of the workgroup's rows, scaled by 64^-0.5 * log2(e), as fp32 in LDS: row r, head hh, piece sb at
  // r * Cc + hh * 64 + ((sb ^ (hh & 7)) * 8)
  const int pieces = Cc / BX_EPL;
  for (int i = tid; i < RB * pieces; i += BX_THREADS) {
    const int r = i / pieces, pc = i % pieces, hh = pc >> 3, sb = pc & 7;
    float v[BX_EPL];
#pragma unroll
    for (int e = 0; e < BX_EPL; ++e) v[e] = 0.f;
    if (r < nr) {
      load8f<T>(q + (row0 + r) * q_ld + h0 * BX_HD + pc * BX_EPL, v);
#pragma unroll
      for (int e = 0; e < BX_EPL; ++e) v[e] *= qscale;
    }
    float* dst = smem + r * Cc + hh * BX_HD + ((sb ^ (hh & 7)) * BX_EPL);
    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
  }
  __syncthreads();

  const int col = (h0 + h) * BX_HD + sub * BX_EPL;
  const T* kvb = kv + (int64_t)sidx * S * kv_ld + k_off + col;
  const uint8_t* mb = kpm ? kpm + (int64_t)sidx * S : nullptr;
  const float* ql = smem + h * BX_HD + ((sub ^ (h & 7)) * BX_EPL);
  float* pb = probs ? probs + row0 * p_row + (int64_t)(h0 + h) * p_head : nullptr;

  float m[RB], l[RB], acc[RB][BX_EPL];
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int e = 0; e < BX_EPL; ++e) acc[r][e] = 0.f;
  }
  // K / V of the pass after this one are in flight while this one is computed
  float kf[BX_EPL], vf[BX_EPL];
#pragma unroll
  for (int e = 0; e < BX_EPL; ++e) { kf[e] = 0.f; vf[e] = 0.f; }
  bool valid = active && j0 + ps < j1 && !(mb && mb[j0 + ps]);
  if (valid) {
    const T* row = kvb + (int64_t)(j0 + ps) * kv_ld;
    load8f<T>(row, kf);
    load8f<T>(row + C, vf);
  }
  for (int jb = j0; jb < j1; jb += P) {
    const int j = jb + ps, jn = j + P;
    const bool on = active && j < j1;
    const bool vnext = active && jn < j1 && !(mb && mb[jn]);
    float kn[BX_EPL], vn[BX_EPL];
#pragma unroll
    for (int e = 0; e < BX_EPL; ++e) { kn[e] = 0.f; vn[e] = 0.f; }
    if (vnext) {
      const T* row = kvb + (int64_t)jn * kv_ld;
      load8f<T>(row, kn);
      load8f<T>(row + C, vn);
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const f32x4 qa = *reinterpret_cast<const f32x4*>(ql + r * Cc);
      const f32x4 qb = *reinterpret_cast<const f32x4*>(ql + r * Cc + 4);
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fmaf(qa[e], kf[e], s);
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fmaf(qb[e], kf[4 + e], s);
      // (every lane of the wave takes part; the 8 lanes of a group share j, so they agree on `valid`)
      s = bx_group_sum(s);
      if (valid) {
        const float mn = fmaxf(m[r], s);
        const float corr = bx_exp2(m[r] - mn), p = bx_exp2(s - mn);
        l[r] = fmaf(l[r], corr, p);
#pragma unroll
        for (int e = 0; e < BX_EPL; ++e) {
          const float a = acc[r][e] * corr;
          acc[r][e] = fmaf(p, vf[e], a);
        }
        m[r] = mn;
      }
      // raw score (-inf at a padded key), normalised below or by the combine kernel
      if (pb && on && sub == 0 && r < nr) pb[(int64_t)r * p_row + j] = valid ? s : -INFINITY;
      // (keeps the scheduler from hoisting the LDS query reads of all 16 rows in front of the first row: 128 more live registers)
      if (r % 4 == 3) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int e = 0; e < BX_EPL; ++e) { kf[e] = kn[e]; vf[e] = vn[e]; }
    valid = vnext;
  }

  // combine the P key lanes of each head through LDS, one row at a time (the query image is no longer needed)
  __syncthreads();
  float* s_m = smem;
  float* s_l = smem + BX_GROUPS;
  float* s_M = smem + 2 * BX_GROUPS;
  float* s_L = smem + 3 * BX_GROUPS;
  float* s_acc = smem + 4 * BX_GROUPS;          // P * Cc = (32 / Hc) * Hc * 64 <= 32 * 64
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (active) {
      if (sub == 0) { s_m[ps * Hc + h] = m[r]; s_l[ps * Hc + h] = l[r]; }
      float* dst = s_acc + ps * Cc + h * BX_HD + sub * BX_EPL;
      *reinterpret_cast<f32x4*>(dst) = f32x4{acc[r][0], acc[r][1], acc[r][2], acc[r][3]};
      *reinterpret_cast<f32x4*>(dst + 4) = f32x4{acc[r][4], acc[r][5], acc[r][6], acc[r][7]};
    }
    __syncthreads();
    if (r < nr) {
      for (int c = tid; c < Cc; c += BX_THREADS) {
        const int hh = c / BX_HD;
        float M = -INFINITY;
        for (int p = 0; p < P; ++p) M = fmaxf(M, s_m[p * Hc + hh]);
        float L = 0.f, A = 0.f;
        if (M != -INFINITY) {
          for (int p = 0; p < P; ++p) {
            const float w = bx_exp2(s_m[p * Hc + hh] - M);
            L = fmaf(w, s_l[p * Hc + hh], L);
            A = fmaf(w, s_acc[p * Cc + c], A);
          }
        }
        if (ws == nullptr) {
          ctx[(row0 + r) * ctx_ld + h0 * BX_HD + c] = Elem<T>::from_f(A / L);
          if (c % BX_HD == 0) { s_M[hh] = M; s_L[hh] = L; }
        } else {
          float* w = ws + ((row0 + r) * nsplit + split) * (2 * H + C);
          if (c % BX_HD == 0) { w[h0 + hh] = M; w[H + h0 + hh] = L; }
          w[2 * H + h0 * BX_HD + c] = A;
        }
      }
    }
    if (ws == nullptr && pb) {
      __syncthreads();
      if (active && sub == 0 && r < nr) {
        const float M = s_M[h], L = s_L[h];
        float* pr = pb + (int64_t)r * p_row;
        for (int j = j0 + ps; j < j1; j += P) pr[j] = bx_exp2(pr[j] - M) / L;   // each lane re-reads only what it wrote
      }
    }
    __syncthreads();
  }
}

// grid (H, rows), 64 threads = the 64 context columns of one head of one row: ctx[r, c] = sum_s 2^(M_s - M) A_s / sum_s 2^(M_s - M) L_s
// over the nsplit partial states of row r in range order; then the head's record entries are normalised.
template <typename T>
__global__ void __launch_bounds__(64) beam_cross_combine_kernel(const float* __restrict__ ws, const int32_t* __restrict__ sent, int n_sent,
                                                               int beam, int nsplit, int S, int H, T* __restrict__ ctx, int64_t ctx_ld,
                                                               float* __restrict__ probs, int64_t p_row, int64_t p_head) {
  const int h = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const int C = H * BX_HD, c = h * BX_HD + tid;
  const int sidx = sent[r / beam];
  float* pr = probs ? probs + (int64_t)r * p_row + (int64_t)h * p_head : nullptr;
  if (sidx < 0 || sidx >= n_sent) {
    ctx[(int64_t)r * ctx_ld + c] = Elem<T>::from_f(NAN);
    if (pr)
      for (int j = tid; j < S; j += 64) pr[j] = NAN;
    return;
  }
  const int64_t stride = 2 * H + C;
  const float* base = ws + (int64_t)r * nsplit * stride;
  float M = -INFINITY;
#pragma unroll 8
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, base[s * stride + h]);
  float L = 0.f, A = 0.f;
  if (M != -INFINITY) {
#pragma unroll 8
    for (int s = 0; s < nsplit; ++s) {
      const float* w = base + s * stride;
      const float ms = w[h];
      const float e = ms == -INFINITY ? 0.f : bx_exp2(ms - M);   // (a range without valid keys adds 0)
      L = fmaf(e, w[H + h], L);
      A = fmaf(e, w[2 * H + c], A);
    }
  }
  ctx[(int64_t)r * ctx_ld + c] = Elem<T>::from_f(A / L);
  if (pr)
    for (int j = tid; j < S; j += 64) pr[j] = bx_exp2(pr[j] - M) / L;
}

template <typename T, int RB>
int launch_beam(const void* q, int64_t q_ld, const void* kv, int64_t kv_ld, int64_t k_off, const uint8_t* kpm, const int32_t* sent,
                int n_sent, int n_live, int beam, int S, int H, void* ctx, int64_t ctx_ld, float* probs, int64_t p_row, int64_t p_head,
                float* ws, hipStream_t st) {
  const int nsplit = bx_splits(S);
  const int chunk = (S + nsplit - 1) / nsplit;
  const int nhc = (H + BX_GROUPS - 1) / BX_GROUPS;
  const int ngrp = (beam + RB - 1) / RB;
  if ((int64_t)ngrp * nhc > 65535) return ST5_ERR_ARG;
  const int hc = H < BX_GROUPS ? H : BX_GROUPS;
  const int img = RB * hc * BX_HD;
  const size_t lds = sizeof(float) * (size_t)(img > BX_COMB_FLOATS ? img : BX_COMB_FLOATS);
  const float qscale = BX_LOG2E / sqrtf((float)BX_HD);
  hipLaunchKernelGGL((beam_cross_attn_kernel<T, RB>), dim3(nsplit, n_live, ngrp * nhc), dim3(BX_THREADS), lds, st,
                     static_cast<const T*>(q), q_ld, static_cast<const T*>(kv), kv_ld, k_off, kpm, sent, n_sent, beam, S, H, chunk, qscale,
                     static_cast<T*>(ctx), ctx_ld, probs, p_row, p_head, nsplit > 1 ? ws : nullptr, nhc);
  if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  if (nsplit > 1) {
    hipLaunchKernelGGL((beam_cross_combine_kernel<T>), dim3(H, n_live * beam), dim3(64), 0, st, ws, sent, n_sent, beam, nsplit, S, H,
                       static_cast<T*>(ctx), ctx_ld, probs, p_row, p_head);
    if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  }
  return ST5_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int64_t st5_beam_cross_attn_ws_bytes(int32_t rows, int32_t S, int32_t H, int32_t head_dim) {
  if (rows <= 0 || S <= 0 || H <= 0 || head_dim <= 0) return 0;
  const int nsplit = bx_splits(S);
  return nsplit > 1 ? (int64_t)rows * nsplit * (2 * H + (int64_t)H * head_dim) * 4 : 0;
}

extern "C" int st5_beam_cross_attn(const void* q, int64_t q_ld, const void* kv, int64_t kv_ld, int64_t k_off, const uint8_t* kpm,
                                   const int32_t* sent, int32_t n_sent, int32_t n_live, int32_t beam, int32_t S, int32_t H,
                                   int32_t head_dim, void* ctx, int64_t ctx_ld, float* probs, int64_t p_row, int64_t p_head, float* ws,
                                   int dtype, void* stream) {
  if (!q || !kv || !ctx || !sent) return ST5_ERR_ARG;
  if (head_dim != BX_HD) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (n_sent <= 0 || n_live <= 0 || n_live > 65535 || beam <= 0 || S <= 0 || H <= 0 || H > 64) return ST5_ERR_ARG;
  if ((int64_t)n_live * beam > 65535) return ST5_ERR_ARG;
  const int64_t C = (int64_t)H * head_dim;
  if (q_ld < C || ctx_ld < C || k_off < 0 || kv_ld < k_off + 2 * C) return ST5_ERR_ARG;
  if (probs && (p_head < S || p_row < (int64_t)H * p_head)) return ST5_ERR_ARG;
  if (bx_splits(S) > 1 && !ws) return ST5_ERR_ARG;
  const int64_t vec = dtype == ST5_F32 ? 4 : 8;   // 16-byte rows: every lane's loads stay aligned
  if (!aligned16(q) || !aligned16(kv) || q_ld % vec || kv_ld % vec || k_off % vec || (ws && !aligned16(ws))) return ST5_ERR_ALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define ST5_BX(T, RB) \
  launch_beam<T, RB>(q, q_ld, kv, kv_ld, k_off, kpm, sent, n_sent, n_live, beam, S, H, ctx, ctx_ld, probs, p_row, p_head, ws, st)
#define ST5_BX_ROWS(T)                    \
  switch (bx_rows_per_block(H, beam)) {   \
    case 1: return ST5_BX(T, 1);          \
    case 2: return ST5_BX(T, 2);          \
    case 4: return ST5_BX(T, 4);          \
    case 8: return ST5_BX(T, 8);          \
    default: return ST5_BX(T, 16);        \
  }
  if (dtype == ST5_F32) { ST5_BX_ROWS(float) }
  ST5_BX_ROWS(bf16_t)
#undef ST5_BX_ROWS
#undef ST5_BX
}
