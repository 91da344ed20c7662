// Ragged (packed) batches of the text-to-waveform path: B utterances lie one after another along time with a zero gap of G mel
// frames after each (speecht5_amd/ragged.py).  At a stage whose cumulative upsampling rate is s, mel frame f
// covers rows [s * f, s * (f + 1)).  The rule that makes every row equal to its single-row result is that every buffer a
// convolution reads holds zeros in its gap rows; the kernels here carry that rule, so no GEMM / convolution kernel knows of it:
//   ragged_pad_act_kernel    the padded act(x) a convolution reads, gap rows SELECTED to zero (never multiplied: whatever a
//                            producer left there, finite or not, does not reach the output)
//   ragged_zero_gaps_kernel  zero the gap rows of a buffer that a convolution / BatchNorm epilogue wrote, launched over the gap
//                            rows only
//   ragged_gather_rows       pack (fp32 records -> packed compute-dtype rows, gap rows zero) and unpack (packed rows -> fp32)
// All offsets are 64-bit: the last generator stage holds 8192 elements per mel frame.
#include "common.h"
#include "../../include/speecht5_hip.h"

#define DISPATCH(dtype, CALL_BF, CALL_F)   \
  if (dtype == ST5_BF16) { CALL_BF; }      \
  else if (dtype == ST5_F32) { CALL_F; }   \
  else return ST5_ERR_ARG;

namespace {

inline dim3 grid_for(long long n) {
  long long b = (n + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

template <int BYTES> struct Chunk;
template <> struct Chunk<16> { typedef uint4 type; __device__ static uint4 zero() { return make_uint4(0u, 0u, 0u, 0u); } };
template <> struct Chunk<4> { typedef uint32_t type; __device__ static uint32_t zero() { return 0u; } };
template <> struct Chunk<2> { typedef uint16_t type; __device__ static uint16_t zero() { return 0; } };

// dst [pad_l + T*s + pad_r, C]: row t' = act(src[t' - pad_l]) where valid[(t' - pad_l) / s], else 0.  One chunk of V elements per
// thread (16 bytes when the rows allow it, one element otherwise).
template <typename T, int V>
__global__ __launch_bounds__(256) void ragged_pad_act_kernel(const T* __restrict__ src, T* __restrict__ dst, const uint8_t* __restrict__ valid,
                                                             long long rows, int s, int C, int pad_l, int pad_r, int act) {
  typedef typename Chunk<V * (int)sizeof(T)>::type W;
  const int cv = C / V;
  const long long n = (rows + pad_l + pad_r) * cv;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long row = i / cv;
    const int c = (int)(i - row * cv) * V;
    const long long t = row - pad_l;
    W v = Chunk<V * (int)sizeof(T)>::zero();
    if (t >= 0 && t < rows && valid[t / s]) {
      v = *reinterpret_cast<const W*>(src + t * C + c);
      if (act != ACT_NONE) {
        T* e = reinterpret_cast<T*>(&v);
#pragma unroll
        for (int j = 0; j < V; ++j) e[j] = Elem<T>::from_f(act_f(act, Elem<T>::to_f(e[j])));
      }
    }
    *reinterpret_cast<W*>(dst + row * C + c) = v;
  }
}

// buf [T*s, C] (row 0 = the first row of mel frame 0): rows [s * f, s * (f + 1)) := 0 for the n_gap frames f listed in
// gap_frames.  A listed frame outside [0, T) or marked valid is skipped: a valid row is never written.
template <typename T, int V>
__global__ __launch_bounds__(256) void ragged_zero_gaps_kernel(T* __restrict__ buf, const uint8_t* __restrict__ valid,
                                                               const int32_t* __restrict__ gap_frames, long long n_gap, long long frames,
                                                               int s, int C) {
  typedef typename Chunk<V * (int)sizeof(T)>::type W;
  const int cv = C / V;
  const long long per = (long long)s * cv, n = n_gap * per;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long g = i / per, j = i - g * per;
    const long long f = gap_frames[g];
    if (f < 0 || f >= frames || valid[f]) continue;
    *reinterpret_cast<W*>(buf + f * s * C + j * V) = Chunk<V * (int)sizeof(T)>::zero();
  }
}

// dst[u, 0:w] = src[idx[u], 0:w] converted, or 0 when idx[u] lies outside [0, src_rows)
template <typename S, typename D>
__global__ __launch_bounds__(256) void ragged_gather_rows_kernel(const S* __restrict__ src, const int32_t* __restrict__ idx, D* __restrict__ dst,
                                                                 long long n_rows, long long src_rows, int w) {
  const long long n = n_rows * w;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long u = i / w;
    const int e = (int)(i - u * w);
    const long long r = idx[u];
    float v = 0.f;
    if (r >= 0 && r < src_rows) v = Elem<S>::to_f(src[r * w + e]);
    dst[i] = Elem<D>::from_f(v);
  }
}

inline bool vec16(const void* a, const void* b, int C, int esz) {
  return (C * esz) % 16 == 0 && (((uintptr_t)a | (uintptr_t)b) % 16) == 0;
}

}  // namespace

extern "C" int st5_ragged_pad_act(const void* src, void* dst, const uint8_t* valid, int64_t frames, int32_t s, int32_t C, int32_t pad_l,
                                  int32_t pad_r, int32_t act, int dtype, void* stream) {
  if (!src || !dst || !valid || frames <= 0 || s <= 0 || C <= 0 || pad_l < 0 || pad_r < 0) return ST5_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long long rows = (long long)frames * s;
  const int esz = dtype == ST5_BF16 ? 2 : 4;
  if (vec16(src, dst, C, esz)) {
    const long long n = (rows + pad_l + pad_r) * (C * esz / 16);
    DISPATCH(dtype, hipLaunchKernelGGL((ragged_pad_act_kernel<bf16_t, 8>), grid_for(n), dim3(256), 0, st, (const bf16_t*)src, (bf16_t*)dst, valid, rows, s, C, pad_l, pad_r, act),
             hipLaunchKernelGGL((ragged_pad_act_kernel<float, 4>), grid_for(n), dim3(256), 0, st, (const float*)src, (float*)dst, valid, rows, s, C, pad_l, pad_r, act));
  } else {
    const long long n = (rows + pad_l + pad_r) * C;
    DISPATCH(dtype, hipLaunchKernelGGL((ragged_pad_act_kernel<bf16_t, 1>), grid_for(n), dim3(256), 0, st, (const bf16_t*)src, (bf16_t*)dst, valid, rows, s, C, pad_l, pad_r, act),
             hipLaunchKernelGGL((ragged_pad_act_kernel<float, 1>), grid_for(n), dim3(256), 0, st, (const float*)src, (float*)dst, valid, rows, s, C, pad_l, pad_r, act));
  }
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}

extern "C" int st5_ragged_zero_gaps(void* buf, const uint8_t* valid, const int32_t* gap_frames, int64_t n_gap, int64_t frames, int32_t s,
                                    int32_t C, int dtype, void* stream) {
  if (!buf || !valid || n_gap < 0 || frames <= 0 || s <= 0 || C <= 0 || (n_gap > 0 && !gap_frames)) return ST5_ERR_ARG;
  if (dtype != ST5_BF16 && dtype != ST5_F32) return ST5_ERR_ARG;
  if (n_gap == 0) return ST5_OK;
  hipStream_t st = (hipStream_t)stream;
  const int esz = dtype == ST5_BF16 ? 2 : 4;
  if (vec16(buf, buf, C, esz)) {
    const long long n = (long long)n_gap * s * (C * esz / 16);
    DISPATCH(dtype, hipLaunchKernelGGL((ragged_zero_gaps_kernel<bf16_t, 8>), grid_for(n), dim3(256), 0, st, (bf16_t*)buf, valid, gap_frames, (long long)n_gap, (long long)frames, s, C),
             hipLaunchKernelGGL((ragged_zero_gaps_kernel<float, 4>), grid_for(n), dim3(256), 0, st, (float*)buf, valid, gap_frames, (long long)n_gap, (long long)frames, s, C));
  } else {
    const long long n = (long long)n_gap * s * C;
    DISPATCH(dtype, hipLaunchKernelGGL((ragged_zero_gaps_kernel<bf16_t, 1>), grid_for(n), dim3(256), 0, st, (bf16_t*)buf, valid, gap_frames, (long long)n_gap, (long long)frames, s, C),
             hipLaunchKernelGGL((ragged_zero_gaps_kernel<float, 1>), grid_for(n), dim3(256), 0, st, (float*)buf, valid, gap_frames, (long long)n_gap, (long long)frames, s, C));
  }
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}

extern "C" int st5_ragged_gather_rows(const void* src, const int32_t* idx, void* dst, int64_t n_rows, int64_t src_rows, int32_t w,
                                      int32_t to_f32, int dtype, void* stream) {
  if (!src || !idx || !dst || n_rows < 0 || src_rows < 0 || w <= 0) return ST5_ERR_ARG;
  if (dtype != ST5_BF16 && dtype != ST5_F32) return ST5_ERR_ARG;
  if (n_rows == 0) return ST5_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid = grid_for((long long)n_rows * w);
  if (dtype == ST5_F32)
    hipLaunchKernelGGL((ragged_gather_rows_kernel<float, float>), grid, dim3(256), 0, st, (const float*)src, idx, (float*)dst, (long long)n_rows, (long long)src_rows, w);
  else if (to_f32)
    hipLaunchKernelGGL((ragged_gather_rows_kernel<bf16_t, float>), grid, dim3(256), 0, st, (const bf16_t*)src, idx, (float*)dst, (long long)n_rows, (long long)src_rows, w);
  else
    hipLaunchKernelGGL((ragged_gather_rows_kernel<float, bf16_t>), grid, dim3(256), 0, st, (const float*)src, idx, (bf16_t*)dst, (long long)n_rows, (long long)src_rows, w);
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}
