// Skinny-M GEMM of the decode loops: out[m, n] = epilogue(sum_k x[m, k] * w[n, k] + bias[n]) for 1 <= M <= 32 rows, weights in
// nn.Linear layout [N, K].  A decode step multiplies B <= 32 rows by ~48 weight matrices of 0.1 ... 4.7 MB; the whole cost of such a
// product is reading the weights once, so this is a weight-STREAMING kernel, not a tile kernel:
//   * one lane owns one weight row n (64 rows per wave) and walks its k range with 16-byte loads; the x values of a k chunk are the
//     same for every lane, i.e. wave-uniform: in fp32 they are fetched through the scalar cache and enter the FMAs as scalar operands,
//     in bf16 as one broadcast 16-byte load per row (a single cache line for the whole wave).  A lane keeps one fp32 accumulator per x
//     row, so there is NO cross-lane reduction and every (m, n) sum is one fmaf chain over ascending k: row m of the output depends on
//     row m of x only, bit for bit, for any M and any content of the other rows.
//   * K is cut into `nslices` slices over grid.y and each slice into four sub-ranges over the four waves of a workgroup.  The four
//     waves' sums are added in wave order through LDS; with more than one slice the workgroup leaves its sum in a fp32 workspace and a
//     second kernel adds the slices in slice order and applies the epilogue (the hand-off is the kernel boundary, as in lm_decode.hip;
//     no atomics).  The partition is a function of K alone (sk_plan), so the reduction order is a function of (N, K, dtype).
//   * the inner product runs on the VALU: at M <= 32 the MFMA's 32-row side would be the weight rows and most of the M side padding,
//     and the operand shuffle (weights k-major per lane) would need an LDS round trip that a streaming kernel does not otherwise have.
//     32 FMAs per weight element pair keep the VALU below the weight stream's cost at these sizes.
// Epilogue (fused into the first kernel when nslices == 1): + bias, activation, dropout (seed by value or seed slot, element index
// (row0 + m) * N + n as st5_gemm counts it), + residual, output in the compute dtype or fp32, and an optional DEVICE-side output
// offset out + clamp(*step, 0, step_cap - 1) * step_stride (the K|V projection of a decode step writes slot `step` of the cache), or
// with st5_gemm_skinny_rows one slot per output row, step_rows[row0 + m] (the synthesis stream: every row at its own position).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "../../include/speecht5_hip.h"

namespace {

constexpr int SK_THREADS = 256;
constexpr int SK_WAVES = SK_THREADS / 64;
constexpr int SK_ROWS = 64;          // weight rows per workgroup (one per lane)
constexpr int SK_MAX_M = 32;
constexpr int SK_SLICE_K = 128;      // k per slice the plan aims at (32 per wave)
constexpr int SK_MAX_SLICES = 16;

struct SkPlan { int nslices, kb, kw; };   // slices over grid.y, k per slice (multiple of 32), k per wave (multiple of 8)

__host__ __device__ inline SkPlan sk_plan(int K) {
  int ns = (K + SK_SLICE_K - 1) / SK_SLICE_K;
  if (ns > SK_MAX_SLICES) ns = SK_MAX_SLICES;
  if (ns < 1) ns = 1;
  int kb = (K + ns - 1) / ns;
  kb = (kb + 31) & ~31;
  ns = (K + kb - 1) / kb;
  return SkPlan{ns, kb, kb / SK_WAVES};
}

struct SkEpi {
  const float* bias;
  const void* res;          // compute dtype, or nullptr
  int64_t res_ld;
  void* out;
  int64_t out_ld;
  const int32_t* step;      // nullptr: no offset; with step_rows != 0 an array indexed by the output row (row0 + m)
  int64_t step_stride;
  int32_t step_cap;
  int32_t act, out_f32, row0;
  int32_t step_rows;
  float dropout_p;
  unsigned long long seed;
};

// slot of output row m: the launch's one counter, or with step_rows the row's own (clamped either way)
__device__ __forceinline__ int sk_slot(const SkEpi& ep, int m) {
  int s0 = ep.step_rows ? ep.step[ep.row0 + m] : *ep.step;
  return s0 < 0 ? 0 : (s0 >= ep.step_cap ? ep.step_cap - 1 : s0);   // no address depends on an unchecked value
}

template <typename T>
__device__ __forceinline__ void sk_epilogue(const SkEpi& ep, int m, int n, int N, float s) {
  constexpr bool FASTACT = sizeof(T) == 2;   // bf16 compute mode, as st5_gemm's epilogue
  float v = ep.bias ? s + ep.bias[n] : s;
  if (ep.act != ACT_NONE) v = act_f<FASTACT>(ep.act, v);
  if (ep.dropout_p > 0.f) {
    const unsigned long long idx = (unsigned long long)(ep.row0 + m) * (unsigned long long)N + (unsigned long long)n;
    v *= dropout_scale(ep.seed, idx, dropout_thresh(ep.dropout_p), 1.0f / (1.0f - ep.dropout_p));
  }
  if (ep.res) v += Elem<T>::to_f(static_cast<const T*>(ep.res)[(int64_t)m * ep.res_ld + n]);
  int64_t off = (int64_t)m * ep.out_ld + n;
  if (ep.step) off += (int64_t)sk_slot(ep, m) * ep.step_stride;
  if (ep.out_f32) static_cast<float*>(ep.out)[off] = v;
  else static_cast<T*>(ep.out)[off] = Elem<T>::from_f(v);
}

// grid (ceil(N / 64), nslices).  MB = M rounded up to a compiled row count; rows >= M repeat row M - 1 and are not stored.
template <typename T, int MB>
__global__ void __launch_bounds__(SK_THREADS) skinny_gemm_kernel(const T* __restrict__ x, int64_t x_ld, const T* __restrict__ w,
                                                                int64_t w_ld, int M, int N, int K, int kb, int kw,
                                                                float* __restrict__ ws, SkEpi ep) {
  constexpr int VEC = Elem<T>::VEC;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform: the x loads below stay scalar)
  const int n = blockIdx.x * SK_ROWS + lane;
  const T* wr = w + (int64_t)(n < N ? n : N - 1) * w_ld;
  const int k0 = blockIdx.y * kb + wave * kw;
  const int k1 = min(K, k0 + kw);
  float acc[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) acc[m] = 0.f;
  for (int k = k0; k < k1; k += VEC) {    // (K % VEC == 0: whole 16-byte vectors only)
    float wv[VEC];
    if constexpr (VEC == 8) {
      load8f<T>(wr + k, wv);
    } else {
      const f32x4 a = *reinterpret_cast<const f32x4*>(wr + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) wv[e] = a[e];
    }
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      // (16 rows' x values at a time: more of them in flight than that overflows the scalar registers)
      if (m % 16 == 0 && m > 0) __builtin_amdgcn_sched_barrier(0);
      const T* xr = x + (int64_t)(m < M ? m : M - 1) * x_ld + k;
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[m] = fmaf(Elem<T>::to_f(xr[e]), wv[e], acc[m]);
    }
  }
  __shared__ float red[SK_WAVES * MB * 64];
#pragma unroll
  for (int m = 0; m < MB; ++m) red[(wave * MB + m) * 64 + lane] = acc[m];
  __syncthreads();
  const int nslices = gridDim.y;
  for (int i = threadIdx.x; i < MB * 64; i += SK_THREADS) {
    const int m = i >> 6, l = i & 63;
    const int nn = blockIdx.x * SK_ROWS + l;
    if (m >= M || nn >= N) continue;
    float s = red[m * 64 + l];
#pragma unroll
    for (int wv = 1; wv < SK_WAVES; ++wv) s += red[(wv * MB + m) * 64 + l];
    if (nslices == 1) sk_epilogue<T>(ep, m, nn, N, s);
    else ws[((int64_t)blockIdx.y * SK_MAX_M + m) * N + nn] = s;
  }
}

// one thread per output element: the slices' sums in slice order, then the epilogue
template <typename T>
__global__ void __launch_bounds__(SK_THREADS) skinny_combine_kernel(const float* __restrict__ ws, int M, int N, int nslices, SkEpi ep) {
  const int64_t i = (int64_t)blockIdx.x * SK_THREADS + threadIdx.x;
  if (i >= (int64_t)M * N) return;
  const int m = (int)(i / N), n = (int)(i % N);
  float s = ws[(int64_t)m * N + n];
  for (int sl = 1; sl < nslices; ++sl) s += ws[((int64_t)sl * SK_MAX_M + m) * N + n];
  sk_epilogue<T>(ep, m, n, N, s);
}

template <typename T, int MB>
void launch_mb(const void* x, int64_t x_ld, const void* w, int64_t w_ld, int M, int N, int K, const SkPlan& pl, float* ws, const SkEpi& ep,
               hipStream_t st) {
  hipLaunchKernelGGL((skinny_gemm_kernel<T, MB>), dim3((N + SK_ROWS - 1) / SK_ROWS, pl.nslices), dim3(SK_THREADS), 0, st,
                     static_cast<const T*>(x), x_ld, static_cast<const T*>(w), w_ld, M, N, K, pl.kb, pl.kw, ws, ep);
}

template <typename T>
int launch_skinny(const void* x, int64_t x_ld, const void* w, int64_t w_ld, int M, int N, int K, float* ws, const SkEpi& ep, hipStream_t st) {
  const SkPlan pl = sk_plan(K);
  if (M <= 1) launch_mb<T, 1>(x, x_ld, w, w_ld, M, N, K, pl, ws, ep, st);
  else if (M <= 4) launch_mb<T, 4>(x, x_ld, w, w_ld, M, N, K, pl, ws, ep, st);
  else if (M <= 8) launch_mb<T, 8>(x, x_ld, w, w_ld, M, N, K, pl, ws, ep, st);
  else if (M <= 16) launch_mb<T, 16>(x, x_ld, w, w_ld, M, N, K, pl, ws, ep, st);
  else launch_mb<T, 32>(x, x_ld, w, w_ld, M, N, K, pl, ws, ep, st);
  if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  if (pl.nslices > 1) {
    const int64_t total = (int64_t)M * N;
    hipLaunchKernelGGL((skinny_combine_kernel<T>), dim3((unsigned)((total + SK_THREADS - 1) / SK_THREADS)), dim3(SK_THREADS), 0, st, ws, M, N,
                       pl.nslices, ep);
    if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  }
  return ST5_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int64_t st5_gemm_skinny_ws_bytes(int32_t N, int32_t K) {
  if (N <= 0 || K <= 0) return 0;
  const SkPlan pl = sk_plan(K);
  return pl.nslices > 1 ? (int64_t)pl.nslices * SK_MAX_M * N * 4 : 0;
}

namespace {
int skinny_entry(const void* x, int64_t x_ld, const void* w, int64_t w_ld, const float* bias, const void* res, int64_t res_ld, void* out,
                 int64_t out_ld, int32_t M, int32_t N, int32_t K, int32_t act, float dropout_p, uint64_t seed, int32_t row0, int32_t out_f32,
                 const int32_t* step, int32_t step_rows, int64_t step_stride, int32_t step_cap, float* ws, int dtype, void* stream) {
  if (!x || !w || !out) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (M < 1 || M > SK_MAX_M || N <= 0 || N > 65535 * SK_ROWS || K <= 0 || row0 < 0) return ST5_ERR_ARG;
  if (act != ACT_NONE && act != ACT_GELU && act != ACT_RELU && act != ACT_TANH) return ST5_ERR_ARG;
  if (!(dropout_p >= 0.f) || dropout_p >= 1.f) return ST5_ERR_ARG;
  if (x_ld < K || w_ld < K || out_ld < N || (res && res_ld < N)) return ST5_ERR_ARG;
  if (step && (step_cap <= 0 || step_stride < 0)) return ST5_ERR_ARG;
  if (sk_plan(K).nslices > 1 && !ws) return ST5_ERR_ARG;
  const int64_t vec = dtype == ST5_F32 ? 4 : 8;   // 16-byte vectors of the weight rows
  if (!aligned16(x) || !aligned16(w) || x_ld % vec || w_ld % vec || K % vec) return ST5_ERR_ALIGN;
  SkEpi ep;
  ep.bias = bias; ep.res = res; ep.res_ld = res_ld; ep.out = out; ep.out_ld = out_ld;
  ep.step = step; ep.step_rows = step_rows; ep.step_stride = step_stride; ep.step_cap = step_cap;
  ep.act = act; ep.out_f32 = out_f32; ep.row0 = row0; ep.dropout_p = dropout_p; ep.seed = seed;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == ST5_F32) return launch_skinny<float>(x, x_ld, w, w_ld, M, N, K, ws, ep, st);
  return launch_skinny<bf16_t>(x, x_ld, w, w_ld, M, N, K, ws, ep, st);
}
}  // namespace

extern "C" int st5_gemm_skinny(const void* x, int64_t x_ld, const void* w, int64_t w_ld, const float* bias, const void* res, int64_t res_ld,
                               void* out, int64_t out_ld, int32_t M, int32_t N, int32_t K, int32_t act, float dropout_p, uint64_t seed,
                               int32_t row0, int32_t out_f32, const int32_t* step, int64_t step_stride, int32_t step_cap, float* ws,
                               int dtype, void* stream) {
  return skinny_entry(x, x_ld, w, w_ld, bias, res, res_ld, out, out_ld, M, N, K, act, dropout_p, seed, row0, out_f32, step, 0, step_stride,
                      step_cap, ws, dtype, stream);
}

// The per-row form: row m of the launch lands in slot clamp(step_rows[row0 + m], 0, step_cap - 1).  The same kernels; only the
// epilogue's slot lookup differs, so a row's bits are those of the scalar form at that row's slot.
extern "C" int st5_gemm_skinny_rows(const void* x, int64_t x_ld, const void* w, int64_t w_ld, const float* bias, const void* res,
                                    int64_t res_ld, void* out, int64_t out_ld, int32_t M, int32_t N, int32_t K, int32_t act,
                                    float dropout_p, uint64_t seed, int32_t row0, int32_t out_f32, const int32_t* step_rows,
                                    int64_t step_stride, int32_t step_cap, float* ws, int dtype, void* stream) {
  if (!step_rows) return ST5_ERR_ARG;
  return skinny_entry(x, x_ld, w, w_ld, bias, res, res_ld, out, out_ld, M, N, K, act, dropout_p, seed, row0, out_f32, step_rows, 1,
                      step_stride, step_cap, ws, dtype, stream);
}
