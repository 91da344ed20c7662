// Speaker-identification head (s2c, SpeechT5/speecht5/models/modules/speaker_decoder_postnet.py): the two steps no other entry point
// of the library covers.  The rest of the head reuses st5_gemm (projections), st5_batchnorm_act_* (BatchNorm1d over [B, C] rows),
// st5_norm_rows (F.normalize) and st5_cross_entropy_rows (the loss).
//
// st5_angular_margin_fwd / _bwd: AngularMargin (AM) and AdditiveAngularMargin (AAM) on fp32 cosine logits [B, V] with one int32 target
// per row (-1 = no margin in that row, the row is only scaled).  One thread per element; the target column is the only one whose
// value depends on the margin, so a row needs no reduction.
// st5_time_mean_fwd / _bwd: encoder_out.mean over all T frames (--sid-pooling-layer encoder, speecht5.py:837-838), padded frames
// included, fp32 [B, C] out.  A workgroup owns 64 channels of one batch row; its 4 waves take every 4th frame with a compensated
// (Kahan) fp32 sum and are combined in LDS, so the result does not drift with T (T is ~8000 for a 160 s utterance).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "../../include/speecht5_hip.h"

namespace {

constexpr int SH_THREADS = 256;
constexpr int TM_CH = 64;                    // channels per workgroup (one wave's width)
constexpr int TM_SLICES = SH_THREADS / TM_CH;

struct MarginCfg {
  int mode;
  float m, s, cos_m, sin_m, th, mm;
};

__device__ __forceinline__ float margin_value(float c, bool tgt, const MarginCfg& k) {
  if (!tgt) return k.s * c;
  if (k.mode == ST5_MARGIN_AM) return k.s * (c - k.m);
  const float sine = sqrtf(fminf(fmaxf(1.0f - c * c, 0.0f), 1.0f));
  const float phi = c * k.cos_m - sine * k.sin_m;
  if (k.mode == ST5_MARGIN_AAM_EASY) return k.s * (c > 0.0f ? phi : c);
  return k.s * (c > k.th ? phi : c - k.mm);
}

// d value / d c.  On the phi branch: cos_m + sin_m * c / sine while 0 < 1 - c^2 < 1; where the clamp is active (|c| >= 1, sine = 0)
// the sine term contributes 0, so the gradient there is s * cos_m (finite; the reference's autograd gives inf / NaN at |c| = 1).
__device__ __forceinline__ float margin_grad(float c, bool tgt, const MarginCfg& k) {
  if (!tgt || k.mode == ST5_MARGIN_AM) return k.s;
  const bool on_phi = k.mode == ST5_MARGIN_AAM_EASY ? c > 0.0f : c > k.th;
  if (!on_phi) return k.s;
  const float u = 1.0f - c * c;
  const float dsine_term = (u > 0.0f && u < 1.0f) ? k.sin_m * c / sqrtf(u) : 0.0f;
  return k.s * (k.cos_m + dsine_term);
}

__global__ void __launch_bounds__(SH_THREADS) margin_fwd_kernel(const float* __restrict__ cosv, int64_t ld, const int32_t* __restrict__ target,
                                                                 float* out, int64_t out_ld, int V, MarginCfg k) {
  const int b = blockIdx.y;
  const int v = blockIdx.x * SH_THREADS + threadIdx.x;
  if (v >= V) return;
  const int t = target[b];
  const float c = cosv[(int64_t)b * ld + v];
  out[(int64_t)b * out_ld + v] = margin_value(c, v == t, k);
}

// dcos columns V..dcos_ld-1 are written as zero: a padded dcos is a GEMM operand as it stands
__global__ void __launch_bounds__(SH_THREADS) margin_bwd_kernel(const float* __restrict__ cosv, int64_t ld, const int32_t* __restrict__ target,
                                                                 const float* dy, int64_t dy_ld, float* dcos, int64_t dcos_ld, int V,
                                                                 MarginCfg k) {
  const int b = blockIdx.y;
  const int v = blockIdx.x * SH_THREADS + threadIdx.x;
  if (v >= dcos_ld) return;
  float g = 0.0f;
  if (v < V) {
    const float c = cosv[(int64_t)b * ld + v];
    g = dy[(int64_t)b * dy_ld + v] * margin_grad(c, v == target[b], k);
  }
  dcos[(int64_t)b * dcos_ld + v] = g;
}

template <typename T>
__global__ void __launch_bounds__(SH_THREADS) time_mean_fwd_kernel(const T* __restrict__ x, int64_t t_stride, int64_t b_stride, int Tn,
                                                                    int C, float inv_T, float* __restrict__ y) {
  __shared__ float part[TM_SLICES][TM_CH];
  const int b = blockIdx.y;
  const int lane = threadIdx.x % TM_CH, slice = threadIdx.x / TM_CH;
  const int c = blockIdx.x * TM_CH + lane;
  float sum = 0.0f, comp = 0.0f;
  if (c < C) {
    const T* p = x + (int64_t)b * b_stride + c;
    for (int t = slice; t < Tn; t += TM_SLICES) {
      const float v = Elem<T>::to_f(p[(int64_t)t * t_stride]) - comp;
      const float s2 = sum + v;
      comp = (s2 - sum) - v;
      sum = s2;
    }
  }
  part[slice][lane] = sum;
  __syncthreads();
  if (slice == 0 && c < C) {
    float tot = part[0][lane];
#pragma unroll
    for (int i = 1; i < TM_SLICES; ++i) tot += part[i][lane];
    y[(int64_t)b * C + c] = tot * inv_T;
  }
}

// dx[t, b, c] (= or +=) dy[b, c] / T, dx time-major [T, B, C] contiguous
template <typename T>
__global__ void __launch_bounds__(SH_THREADS) time_mean_bwd_kernel(const float* __restrict__ dy, int64_t BC, int64_t n, float inv_T,
                                                                    int accumulate, T* __restrict__ dx) {
  const int64_t stride = (int64_t)gridDim.x * SH_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * SH_THREADS + threadIdx.x; i < n; i += stride) {
    float g = dy[i % BC] * inv_T;
    if (accumulate) g += Elem<T>::to_f(dx[i]);
    dx[i] = Elem<T>::from_f(g);
  }
}

bool margin_cfg(int mode, float margin, float scale, MarginCfg* k) {
  if (mode != ST5_MARGIN_AM && mode != ST5_MARGIN_AAM && mode != ST5_MARGIN_AAM_EASY) return false;
  // the constants of AdditiveAngularMargin.__init__, in double then rounded once (math.cos / math.sin there)
  const double m = margin;
  *k = MarginCfg{mode, margin, scale, (float)cos(m), (float)sin(m), (float)cos(M_PI - m), (float)(sin(M_PI - m) * m)};
  return true;
}

}  // namespace

extern "C" int st5_angular_margin_fwd(const float* cosv, int64_t ld, const int32_t* target, float* out, int64_t out_ld, int32_t B, int32_t V,
                                      int32_t mode, float margin, float scale, void* stream) {
  MarginCfg k;
  if (!cosv || !target || !out || B < 0 || B > 65535 || V <= 0 || ld < V || out_ld < V || !margin_cfg(mode, margin, scale, &k))
    return ST5_ERR_ARG;
  if (B == 0) return ST5_OK;
  hipLaunchKernelGGL(margin_fwd_kernel, dim3((V + SH_THREADS - 1) / SH_THREADS, B), dim3(SH_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), cosv, ld, target, out, out_ld, V, k);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_angular_margin_bwd(const float* cosv, int64_t ld, const int32_t* target, const float* dy, int64_t dy_ld, float* dcos,
                                      int64_t dcos_ld, int32_t B, int32_t V, int32_t mode, float margin, float scale, void* stream) {
  MarginCfg k;
  if (!cosv || !target || !dy || !dcos || B < 0 || B > 65535 || V <= 0 || ld < V || dy_ld < V || dcos_ld < V ||
      dcos_ld > (int64_t)1 << 30 || !margin_cfg(mode, margin, scale, &k))
    return ST5_ERR_ARG;
  if (B == 0) return ST5_OK;
  hipLaunchKernelGGL(margin_bwd_kernel, dim3((unsigned)((dcos_ld + SH_THREADS - 1) / SH_THREADS), B), dim3(SH_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), cosv, ld, target, dy, dy_ld, dcos, dcos_ld, V, k);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_time_mean_fwd(const void* x, int64_t t_stride, int64_t b_stride, int32_t T, int32_t B, int32_t C, float* y, int dtype,
                                 void* stream) {
  if (!x || !y || T <= 0 || B < 0 || B > 65535 || C <= 0 || t_stride < 0 || b_stride < 0) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  if (B == 0) return ST5_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((C + TM_CH - 1) / TM_CH, B);
  const float inv_T = 1.0f / (float)T;
  if (dtype == ST5_F32)
    hipLaunchKernelGGL(time_mean_fwd_kernel<float>, grid, dim3(SH_THREADS), 0, st, static_cast<const float*>(x), t_stride, b_stride, T, C,
                       inv_T, y);
  else
    hipLaunchKernelGGL(time_mean_fwd_kernel<bf16_t>, grid, dim3(SH_THREADS), 0, st, static_cast<const bf16_t*>(x), t_stride, b_stride, T,
                       C, inv_T, y);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_time_mean_bwd(const float* dy, int32_t T, int32_t B, int32_t C, int32_t accumulate, void* dx, int dtype, void* stream) {
  if (!dy || !dx || T <= 0 || B < 0 || C <= 0) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  const int64_t BC = (int64_t)B * C, n = BC * T;
  if (n == 0) return ST5_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t want = (n + SH_THREADS - 1) / SH_THREADS;
  const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);
  const float inv_T = 1.0f / (float)T;
  if (dtype == ST5_F32)
    hipLaunchKernelGGL(time_mean_bwd_kernel<float>, dim3(blocks), dim3(SH_THREADS), 0, st, dy, BC, n, inv_T, accumulate,
                       static_cast<float*>(dx));
  else
    hipLaunchKernelGGL(time_mean_bwd_kernel<bf16_t>, dim3(blocks), dim3(SH_THREADS), 0, st, dy, BC, n, inv_T, accumulate,
                       static_cast<bf16_t*>(dx));
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}
