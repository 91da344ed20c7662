// Incremental decoding of the shallow-fusion language model (arch transformer_lm_t5) inside ASR beam search.
// The reference re-runs the whole prefix through the LM at every step (SpeechT5/speecht5/sequence_generator.py:420-425:
// lm_model(tokens[:, :step + 1])); here every layer keeps the projected keys / values of every position once, in a SLOT
// cache, and one query per hypothesis row attends over its ancestry:
//   kv  [rows_cap, Tmax, 2C] per layer (compute dtype): slot (r, j) = [k | v] that hypothesis row r produced at position j;
//   anc [rows, Tmax] int32 (one table for all layers): row r reads position j from slot (anc[r, j], j).
// A slot is written exactly once, at the step equal to its position, so a beam reorder only gathers the int32 table
// (st5_lm_reorder) and never moves a key or a value -- also when several rows share a parent or the batch shrinks.
//
// st5_lm_decode_attn: ctx[r, h*hd:(h+1)*hd] = softmax(q_h . K_h^T * hd^-0.5) . V_h over positions 0..t-1, fp32 accumulation,
// online softmax.  A workgroup takes one row and a range of positions, ALL heads: groups of 4 lanes own one (position, head)
// pair, so a wave reads whole contiguous position rows (all heads of a position in one gather).  Once t > LM_SPLIT_MIN the
// position range is split over several workgroups (rows x heads alone is 80 workgroups for beam 5) and a second kernel combines
// the partial (max, sum, acc) states: the hand-off between workgroups is the kernel boundary, no in-launch protocol.
// st5_lm_fuse_logprobs: lprobs[r, :V_lm] += w * log_softmax(logits[r, :V_lm]) (sequence_generator.py:420-425), fp32.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "../../include/speecht5_hip.h"

namespace {

constexpr int LM_THREADS = 256;
constexpr int LM_GROUPS = LM_THREADS / 4;   // 4 lanes per (position, head)
constexpr int LM_SPLIT_MIN = 64;            // up to this many positions one workgroup per row covers them all
constexpr int LM_SPLIT_CHUNK = 16;          // fewest positions per workgroup once split
constexpr int LM_SPLIT_MAX = 128;
constexpr int LM_TARGET_BLOCKS = 1024;      // 4 workgroups per CU

__host__ __device__ inline int lm_splits(int rows, int t) {
  if (t <= LM_SPLIT_MIN) return 1;
  int want = (LM_TARGET_BLOCKS + rows - 1) / rows;
  const int most = (t + LM_SPLIT_CHUNK - 1) / LM_SPLIT_CHUNK;
  if (want > most) want = most;
  if (want > LM_SPLIT_MAX) want = LM_SPLIT_MAX;
  return want < 2 ? 2 : want;
}

// 4 consecutive elements as floats (fp32: one 16-byte load; bf16: one 8-byte load)
__device__ __forceinline__ void load4f(const float* p, float* v) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
}
__device__ __forceinline__ void load4f(const bf16_t* p, float* v) {
  const u32x2 a = *reinterpret_cast<const u32x2*>(p);
  v[0] = __uint_as_float(a[0] << 16); v[1] = __uint_as_float(a[0] & 0xffff0000u);
  v[2] = __uint_as_float(a[1] << 16); v[3] = __uint_as_float(a[1] & 0xffff0000u);
}

// grid (nsplit, rows).  ws == nullptr (nsplit 1): ctx is written directly.  Otherwise ws holds per (row, split): H maxima, H sums,
// then the C unnormalised accumulators.
template <typename T, int HD>
__device__ __forceinline__ void lm_decode_attn_body(
    const T* __restrict__ q, int64_t q_ld, const T* __restrict__ kv, int Tmax, int rows_cap, const int32_t* __restrict__ anc,
    int64_t anc_ld, int t, int H, int chunk, float scale, T* __restrict__ ctx, int64_t ctx_ld, float* __restrict__ ws, const int r,
    const int split, const int nsplit, const int ws_ld) {   // ws_ld: split states per row in ws (nsplit, or the grid's with per-row t)
  constexpr int EPL = HD / 4;                // elements per lane: 20 (hd 80) or 16 (hd 64)
  const int C = H * HD;
  const int tid = threadIdx.x, g = tid >> 2, sub = tid & 3;
  const int P = LM_GROUPS / H;                // positions in flight per pass
  const int h = g % H, ps = g / H;
  const bool active = ps < P;
  const int j0 = split * chunk;
  const int j1 = min(t, j0 + chunk);
  const int col = h * HD + sub * EPL;

  float qf[EPL], acc[EPL];
  float m = -INFINITY, l = 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
  if (active) {
#pragma unroll
    for (int e = 0; e < EPL; e += 4) load4f(q + (int64_t)r * q_ld + col + e, qf + e);
#pragma unroll
    for (int e = 0; e < EPL; ++e) qf[e] *= scale;
  }
  const int64_t row_stride = (int64_t)Tmax * 2 * C;
  for (int jb = j0; jb < j1; jb += P) {
    const int j = jb + ps;
    const bool on = active && j < j1;
    float kf[EPL], vf[EPL];
    float s = -INFINITY;
    if (on) {
      const int slot = anc[(int64_t)r * anc_ld + j];
      if (slot >= 0 && slot < rows_cap) {
        const T* base = kv + (int64_t)slot * row_stride + (int64_t)j * 2 * C + col;
#pragma unroll
        for (int e = 0; e < EPL; e += 4) { load4f(base + e, kf + e); load4f(base + C + e, vf + e); }
        s = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) s = fmaf(qf[e], kf[e], s);
      } else {
        s = NAN;                              // a broken ancestry entry shows up in the output, it is never dereferenced
#pragma unroll
        for (int e = 0; e < EPL; ++e) vf[e] = NAN;
      }
    }
    // (every lane of the wave takes part in the 4-lane sum; inactive groups add -inf / NaN among themselves only)
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (on) {
      const float mn = fmaxf(m, s);
      const float corr = expf(m - mn), p = expf(s - mn);
      l = l * corr + p;
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[e] = fmaf(p, vf[e], acc[e] * corr);
      m = mn;
      if (s != s) m = s;                      // (fmaxf drops a NaN score: keep it)
    }
  }

  // combine the P position lanes of each head through LDS
  __shared__ float s_m[LM_GROUPS], s_l[LM_GROUPS];
  __shared__ float s_acc[LM_GROUPS * HD];      // P * C = (64 / H) * H * HD <= 64 * HD
  if (active) {
    if (sub == 0) { s_m[ps * H + h] = m; s_l[ps * H + h] = l; }
#pragma unroll
    for (int e = 0; e < EPL; ++e) s_acc[ps * C + col + e] = acc[e];
  }
  __syncthreads();
  for (int c = tid; c < C; c += LM_THREADS) {
    const int hh = c / HD;
    float M = -INFINITY;
    bool nan = false;
    for (int p = 0; p < P; ++p) { const float mp = s_m[p * H + hh]; M = fmaxf(M, mp); nan |= mp != mp; }
    float L = 0.f, A = 0.f;
    if (nan) { L = NAN; A = NAN; }
    else if (M != -INFINITY) {
      for (int p = 0; p < P; ++p) {
        const float w = expf(s_m[p * H + hh] - M);
        L = fmaf(w, s_l[p * H + hh], L);
        A = fmaf(w, s_acc[p * C + c], A);
      }
    }
    if (ws == nullptr) {
      ctx[(int64_t)r * ctx_ld + c] = Elem<T>::from_f(A / L);
    } else {
      float* w = ws + ((int64_t)r * ws_ld + split) * (2 * H + C);
      if (c % HD == 0) { w[hh] = M; w[H + hh] = L; }
      w[2 * H + c] = A;
    }
  }
}

template <typename T, int HD>
__global__ void __launch_bounds__(LM_THREADS) lm_decode_attn_kernel(
    const T* __restrict__ q, int64_t q_ld, const T* __restrict__ kv, int Tmax, int rows_cap, const int32_t* __restrict__ anc,
    int64_t anc_ld, int t, int H, int chunk, float scale, T* __restrict__ ctx, int64_t ctx_ld, float* __restrict__ ws) {
  lm_decode_attn_body<T, HD>(q, q_ld, kv, Tmax, rows_cap, anc, anc_ld, t, H, chunk, scale, ctx, ctx_ld, ws, blockIdx.y, blockIdx.x,
                             gridDim.x, gridDim.x);
}

// The same launch with t read from device memory (a decode step replayed from a graph): t = clamp(*step + t_add, 1, t_max); the grid is
// sized for t_max (grid.x = lm_splits(rows, t_max), which bounds lm_splits(rows, t) for every t <= t_max); the partition of the key
// range is the host launch's function of (rows, t), evaluated here, and workgroups past it exit at once.
__device__ __forceinline__ int lm_dev_t(const int32_t* step, int t_add, int t_max) {
  const int t = *step + t_add;
  return t < 1 ? 1 : (t > t_max ? t_max : t);
}
template <typename T, int HD>
__global__ void __launch_bounds__(LM_THREADS) lm_decode_attn_dev_kernel(
    const T* __restrict__ q, int64_t q_ld, const T* __restrict__ kv, int Tmax, int rows_cap, const int32_t* __restrict__ anc,
    int64_t anc_ld, const int32_t* __restrict__ step, int t_add, int t_max, int H, float scale, T* __restrict__ ctx, int64_t ctx_ld,
    float* __restrict__ ws) {
  const int t = lm_dev_t(step, t_add, t_max);
  const int nsplit = lm_splits((int)gridDim.y, t);
  if ((int)blockIdx.x >= nsplit) return;
  const int chunk = (t + nsplit - 1) / nsplit;
  lm_decode_attn_body<T, HD>(q, q_ld, kv, Tmax, rows_cap, anc, anc_ld, t, H, chunk, scale, ctx, ctx_ld, nsplit > 1 ? ws : nullptr,
                             blockIdx.y, blockIdx.x, nsplit, nsplit);
}
// The same with one position per row: t_b = clamp(pos[b] + t_add, 1, t_max), read once per workgroup through the scalar cache
// (blockIdx.y is uniform, so is t).  Rows differ in their split count, so a row's states sit at the GRID's stride in ws (row b
// owns ws[b * gridDim.x ...]): no two rows' regions overlap whatever their positions.  Where the states sit does not enter the bits.
template <typename T, int HD>
__global__ void __launch_bounds__(LM_THREADS) lm_decode_attn_rows_kernel(
    const T* __restrict__ q, int64_t q_ld, const T* __restrict__ kv, int Tmax, int rows_cap, const int32_t* __restrict__ anc,
    int64_t anc_ld, const int32_t* __restrict__ pos, int t_add, int t_max, int H, float scale, T* __restrict__ ctx, int64_t ctx_ld,
    float* __restrict__ ws) {
  const int t = lm_dev_t(pos + blockIdx.y, t_add, t_max);
  const int nsplit = lm_splits((int)gridDim.y, t);
  if ((int)blockIdx.x >= nsplit) return;
  const int chunk = (t + nsplit - 1) / nsplit;
  lm_decode_attn_body<T, HD>(q, q_ld, kv, Tmax, rows_cap, anc, anc_ld, t, H, chunk, scale, ctx, ctx_ld, nsplit > 1 ? ws : nullptr,
                             blockIdx.y, blockIdx.x, nsplit, gridDim.x);
}

// grid (C / 64, rows), one thread per output column: ctx[r, c] = sum_s e^(M_s - M) A_s / sum_s e^(M_s - M) L_s over the nsplit
// partial states of row r.  (One column per thread keeps the nsplit loads of a thread independent of each other; a workgroup per
// row that walked its columns in turn took ~100 us per launch at 5 rows.)
template <typename T>
__device__ __forceinline__ void lm_decode_combine_body(const float* __restrict__ ws, int nsplit, int H, int HD, T* __restrict__ ctx,
                                                       int64_t ctx_ld, int ws_ld) {
  const int r = blockIdx.y, C = H * HD;
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const int h = c / HD;
  const int64_t stride = 2 * H + C;
  const float* base = ws + (int64_t)r * ws_ld * stride;
  float M = -INFINITY;
  bool nan = false;
#pragma unroll 8
  for (int s = 0; s < nsplit; ++s) { const float ms = base[s * stride + h]; M = fmaxf(M, ms); nan |= ms != ms; }
  float L = 0.f, A = 0.f;
  if (nan) { L = NAN; A = NAN; }
  else {
#pragma unroll 8
    for (int s = 0; s < nsplit; ++s) {
      const float* w = base + s * stride;
      const float ms = w[h];
      const float e = ms == -INFINITY ? 0.f : expf(ms - M);    // (a split without positions)
      L = fmaf(e, w[H + h], L);
      A = fmaf(e, w[2 * H + c], A);
    }
  }
  ctx[(int64_t)r * ctx_ld + c] = Elem<T>::from_f(A / L);
}
template <typename T>
__global__ void __launch_bounds__(64) lm_decode_combine_kernel(const float* __restrict__ ws, int nsplit, int H, int HD,
                                                              T* __restrict__ ctx, int64_t ctx_ld) {
  lm_decode_combine_body<T>(ws, nsplit, H, HD, ctx, ctx_ld, nsplit);
}
// device-t form: nothing to combine while the step's key range is one workgroup's (the attention kernel wrote ctx itself)
template <typename T>
__global__ void __launch_bounds__(64) lm_decode_combine_dev_kernel(const float* __restrict__ ws, const int32_t* __restrict__ step, int t_add,
                                                                  int t_max, int H, int HD, T* __restrict__ ctx, int64_t ctx_ld) {
  const int nsplit = lm_splits((int)gridDim.y, lm_dev_t(step, t_add, t_max));
  if (nsplit <= 1) return;
  lm_decode_combine_body<T>(ws, nsplit, H, HD, ctx, ctx_ld, nsplit);
}
// per-row form: row r's split count follows its own position; its states sit at the grid's stride (ws_ld = the launch's nsplit)
template <typename T>
__global__ void __launch_bounds__(64) lm_decode_combine_rows_kernel(const float* __restrict__ ws, const int32_t* __restrict__ pos, int t_add,
                                                                   int t_max, int H, int HD, T* __restrict__ ctx, int64_t ctx_ld,
                                                                   int ws_ld) {
  const int nsplit = lm_splits((int)gridDim.y, lm_dev_t(pos + blockIdx.y, t_add, t_max));
  if (nsplit <= 1) return;
  lm_decode_combine_body<T>(ws, nsplit, H, HD, ctx, ctx_ld, ws_ld);
}

// anc_new[r, j] = anc[order[r], j] for j < t, = r for t <= j < Tmax (the row's own slots from position t on); an order entry
// outside [0, rows_old) gives the row -1 everywhere below t, which the attention kernel turns into NaN.
__global__ void lm_reorder_kernel(const int32_t* __restrict__ anc, int64_t anc_ld, const int64_t* __restrict__ order, int rows_old,
                                  int t, int Tmax, int32_t* __restrict__ anc_new, int64_t new_ld) {
  const int r = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Tmax) return;
  const int64_t o = order[r];
  int32_t v = r;
  if (j < t) v = (o >= 0 && o < rows_old) ? anc[o * anc_ld + j] : -1;
  anc_new[(int64_t)r * new_ld + j] = v;
}

template <typename T>
__global__ void __launch_bounds__(LM_THREADS) lm_fuse_logprobs_kernel(float* __restrict__ lprobs, int64_t lp_ld,
                                                                     const T* __restrict__ logits, int64_t lg_ld, int V, float w) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const T* x = logits + (int64_t)r * lg_ld;
  __shared__ float red[LM_THREADS / 64];
  float mx = -INFINITY;
  for (int c = tid; c < V; c += LM_THREADS) mx = fmaxf(mx, Elem<T>::to_f(x[c]));
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int i = 1; i < LM_THREADS / 64; ++i) mx = fmaxf(mx, red[i]);
  __syncthreads();
  float sum = 0.f;
  for (int c = tid; c < V; c += LM_THREADS) sum += expf(Elem<T>::to_f(x[c]) - mx);
  sum = wave_sum(sum);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  sum = 0.f;
#pragma unroll
  for (int i = 0; i < LM_THREADS / 64; ++i) sum += red[i];
  const float lse = logf(sum);
  float* y = lprobs + (int64_t)r * lp_ld;
  for (int c = tid; c < V; c += LM_THREADS) y[c] += ((Elem<T>::to_f(x[c]) - mx) - lse) * w;
}

template <typename T, int HD>
int launch_attn(const void* q, int64_t q_ld, const void* kv, int Tmax, int rows_cap, const int32_t* anc, int64_t anc_ld, int rows,
                int t, int H, void* ctx, int64_t ctx_ld, float* ws, hipStream_t st) {
  const int nsplit = lm_splits(rows, t);
  const int chunk = (t + nsplit - 1) / nsplit;
  const float scale = 1.0f / sqrtf((float)HD);
  hipLaunchKernelGGL((lm_decode_attn_kernel<T, HD>), dim3(nsplit, rows), dim3(LM_THREADS), 0, st, static_cast<const T*>(q), q_ld,
                     static_cast<const T*>(kv), Tmax, rows_cap, anc, anc_ld, t, H, chunk, scale, static_cast<T*>(ctx), ctx_ld,
                     nsplit > 1 ? ws : nullptr);
  if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  if (nsplit > 1) {
    hipLaunchKernelGGL((lm_decode_combine_kernel<T>), dim3((H * HD + 63) / 64, rows), dim3(64), 0, st, ws, nsplit, H, HD,
                       static_cast<T*>(ctx), ctx_ld);
    if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  }
  return ST5_OK;
}

template <typename T, int HD>
int launch_attn_dev(const void* q, int64_t q_ld, const void* kv, int Tmax, int rows_cap, const int32_t* anc, int64_t anc_ld, int rows,
                    const int32_t* step, int t_add, int t_max, int H, void* ctx, int64_t ctx_ld, float* ws, hipStream_t st) {
  const int nsplit = lm_splits(rows, t_max);
  const float scale = 1.0f / sqrtf((float)HD);
  hipLaunchKernelGGL((lm_decode_attn_dev_kernel<T, HD>), dim3(nsplit, rows), dim3(LM_THREADS), 0, st, static_cast<const T*>(q), q_ld,
                     static_cast<const T*>(kv), Tmax, rows_cap, anc, anc_ld, step, t_add, t_max, H, scale, static_cast<T*>(ctx), ctx_ld, ws);
  if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  if (nsplit > 1) {
    hipLaunchKernelGGL((lm_decode_combine_dev_kernel<T>), dim3((H * HD + 63) / 64, rows), dim3(64), 0, st, ws, step, t_add, t_max, H, HD,
                       static_cast<T*>(ctx), ctx_ld);
    if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  }
  return ST5_OK;
}

template <typename T, int HD>
int launch_attn_rows(const void* q, int64_t q_ld, const void* kv, int Tmax, int rows_cap, const int32_t* anc, int64_t anc_ld, int rows,
                     const int32_t* pos, int t_add, int t_max, int H, void* ctx, int64_t ctx_ld, float* ws, hipStream_t st) {
  const int nsplit = lm_splits(rows, t_max);
  const float scale = 1.0f / sqrtf((float)HD);
  hipLaunchKernelGGL((lm_decode_attn_rows_kernel<T, HD>), dim3(nsplit, rows), dim3(LM_THREADS), 0, st, static_cast<const T*>(q), q_ld,
                     static_cast<const T*>(kv), Tmax, rows_cap, anc, anc_ld, pos, t_add, t_max, H, scale, static_cast<T*>(ctx), ctx_ld, ws);
  if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  if (nsplit > 1) {
    hipLaunchKernelGGL((lm_decode_combine_rows_kernel<T>), dim3((H * HD + 63) / 64, rows), dim3(64), 0, st, ws, pos, t_add, t_max, H, HD,
                       static_cast<T*>(ctx), ctx_ld, nsplit);
    if (hipGetLastError() != hipSuccess) return ST5_ERR_LAUNCH;
  }
  return ST5_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int st5_lm_decode_attn_rows(const void* q, int64_t q_ld, const void* kv, int32_t rows_cap, int32_t Tmax, const int32_t* anc,
                                       int64_t anc_ld, int32_t rows, const int32_t* pos, int32_t t_add, int32_t t_max, int32_t H,
                                       int32_t head_dim, void* ctx, int64_t ctx_ld, float* ws, int dtype, void* stream) {
  if (!q || !kv || !anc || !ctx || !pos) return ST5_ERR_ARG;
  if (head_dim != 64 && head_dim != 80) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (rows <= 0 || rows > rows_cap || rows > 65535 || t_max <= 0 || t_max > Tmax || H <= 0 || H > LM_GROUPS) return ST5_ERR_ARG;
  const int64_t C = (int64_t)H * head_dim;
  if (q_ld < C || ctx_ld < C || anc_ld < t_max) return ST5_ERR_ARG;
  if (lm_splits(rows, t_max) > 1 && !ws) return ST5_ERR_ARG;
  const int64_t vec = dtype == ST5_F32 ? 4 : 8;
  if (!aligned16(q) || !aligned16(kv) || q_ld % vec || (ws && !aligned16(ws))) return ST5_ERR_ALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define ST5_LM_ROWS(T, HD) launch_attn_rows<T, HD>(q, q_ld, kv, Tmax, rows_cap, anc, anc_ld, rows, pos, t_add, t_max, H, ctx, ctx_ld, ws, st)
  if (dtype == ST5_F32) return head_dim == 80 ? ST5_LM_ROWS(float, 80) : ST5_LM_ROWS(float, 64);
  return head_dim == 80 ? ST5_LM_ROWS(bf16_t, 80) : ST5_LM_ROWS(bf16_t, 64);
#undef ST5_LM_ROWS
}

extern "C" int64_t st5_lm_decode_attn_ws_bytes(int32_t rows, int32_t t, int32_t H, int32_t head_dim) {
  if (rows <= 0 || t <= 0 || H <= 0 || head_dim <= 0) return 0;
  const int nsplit = lm_splits(rows, t);
  return nsplit > 1 ? (int64_t)rows * nsplit * (2 * H + (int64_t)H * head_dim) * 4 : 0;
}

extern "C" int st5_lm_decode_attn(const void* q, int64_t q_ld, const void* kv, int32_t rows_cap, int32_t Tmax, const int32_t* anc,
                                  int64_t anc_ld, int32_t rows, int32_t t, int32_t H, int32_t head_dim, void* ctx, int64_t ctx_ld,
                                  float* ws, int dtype, void* stream) {
  if (!q || !kv || !anc || !ctx) return ST5_ERR_ARG;
  if (head_dim != 64 && head_dim != 80) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (rows <= 0 || rows > rows_cap || rows > 65535 || t <= 0 || t > Tmax || H <= 0 || H > LM_GROUPS) return ST5_ERR_ARG;
  const int64_t C = (int64_t)H * head_dim;
  if (q_ld < C || ctx_ld < C || anc_ld < t) return ST5_ERR_ARG;
  if (lm_splits(rows, t) > 1 && !ws) return ST5_ERR_ARG;
  const int64_t vec = dtype == ST5_F32 ? 4 : 8;   // 16-byte rows: every lane's 4-element loads stay aligned
  if (!aligned16(q) || !aligned16(kv) || q_ld % vec || (ws && !aligned16(ws))) return ST5_ERR_ALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == ST5_F32)
    return head_dim == 80 ? launch_attn<float, 80>(q, q_ld, kv, Tmax, rows_cap, anc, anc_ld, rows, t, H, ctx, ctx_ld, ws, st)
                          : launch_attn<float, 64>(q, q_ld, kv, Tmax, rows_cap, anc, anc_ld, rows, t, H, ctx, ctx_ld, ws, st);
  return head_dim == 80 ? launch_attn<bf16_t, 80>(q, q_ld, kv, Tmax, rows_cap, anc, anc_ld, rows, t, H, ctx, ctx_ld, ws, st)
                        : launch_attn<bf16_t, 64>(q, q_ld, kv, Tmax, rows_cap, anc, anc_ld, rows, t, H, ctx, ctx_ld, ws, st);
}

extern "C" int st5_lm_decode_attn_dev(const void* q, int64_t q_ld, const void* kv, int32_t rows_cap, int32_t Tmax, const int32_t* anc,
                                      int64_t anc_ld, int32_t rows, const int32_t* step, int32_t t_add, int32_t t_max, int32_t H,
                                      int32_t head_dim, void* ctx, int64_t ctx_ld, float* ws, int dtype, void* stream) {
  if (!q || !kv || !anc || !ctx || !step) return ST5_ERR_ARG;
  if (head_dim != 64 && head_dim != 80) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (rows <= 0 || rows > rows_cap || rows > 65535 || t_max <= 0 || t_max > Tmax || H <= 0 || H > LM_GROUPS) return ST5_ERR_ARG;
  const int64_t C = (int64_t)H * head_dim;
  if (q_ld < C || ctx_ld < C || anc_ld < t_max) return ST5_ERR_ARG;
  if (lm_splits(rows, t_max) > 1 && !ws) return ST5_ERR_ARG;
  const int64_t vec = dtype == ST5_F32 ? 4 : 8;
  if (!aligned16(q) || !aligned16(kv) || q_ld % vec || (ws && !aligned16(ws))) return ST5_ERR_ALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define ST5_LM_DEV(T, HD) launch_attn_dev<T, HD>(q, q_ld, kv, Tmax, rows_cap, anc, anc_ld, rows, step, t_add, t_max, H, ctx, ctx_ld, ws, st)
  if (dtype == ST5_F32) return head_dim == 80 ? ST5_LM_DEV(float, 80) : ST5_LM_DEV(float, 64);
  return head_dim == 80 ? ST5_LM_DEV(bf16_t, 80) : ST5_LM_DEV(bf16_t, 64);
#undef ST5_LM_DEV
}

extern "C" int st5_lm_reorder(const int32_t* anc, int64_t anc_ld, const int64_t* order, int32_t rows_old, int32_t rows_new, int32_t t,
                              int32_t Tmax, int32_t* anc_new, int64_t new_ld, void* stream) {
  if (!anc || !order || !anc_new || anc == anc_new) return ST5_ERR_ARG;
  if (rows_old <= 0 || rows_new <= 0 || rows_new > 65535 || t < 0 || t > Tmax || Tmax <= 0 || anc_ld < Tmax || new_ld < Tmax)
    return ST5_ERR_ARG;
  hipLaunchKernelGGL(lm_reorder_kernel, dim3((Tmax + 255) / 256, rows_new), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), anc,
                     anc_ld, order, rows_old, t, Tmax, anc_new, new_ld);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_lm_fuse_logprobs(float* lprobs, int64_t lp_ld, const void* logits, int64_t lg_ld, int32_t rows, int32_t V_lm,
                                    float lm_weight, int dtype, void* stream) {
  if (!lprobs || !logits || rows < 0 || V_lm <= 0 || lp_ld < V_lm || lg_ld < V_lm) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (rows == 0) return ST5_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == ST5_F32)
    hipLaunchKernelGGL(lm_fuse_logprobs_kernel<float>, dim3(rows), dim3(LM_THREADS), 0, st, lprobs, lp_ld,
                       static_cast<const float*>(logits), lg_ld, V_lm, lm_weight);
  else
    hipLaunchKernelGGL(lm_fuse_logprobs_kernel<bf16_t>, dim3(rows), dim3(LM_THREADS), 0, st, lprobs, lp_ld,
                       static_cast<const bf16_t*>(logits), lg_ld, V_lm, lm_weight);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}
