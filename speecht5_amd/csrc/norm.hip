// LayerNorm forward/backward + column reductions (wave64 row reductions, 16-byte vector IO).
// Replaces fairseq LayerNorm (F.layer_norm) at encoder.py:226-227, transformer_layer.py:124,132,
// 350,378,402, speech_encoder_prenet.py:174 and the bias / affine-parameter gradient reductions
// of their autograd backward passes.  HBM-bound: one read + one write per element in forward;
// backward reads x and dy once for dx and once more for the (deterministic, two-stage)
// dgamma/dbeta column reduction.
#include "common.h"
#include "stream_scratch.h"
#include "../../include/speecht5_hip.h"

namespace {

constexpr int MAXCH = 8;  // up to 8 chunks x 512 columns per wave pass => cols <= 4096 held in registers

template <typename T, int NCH>
__device__ __forceinline__ void load_row(const T* row, int cols, int lane, bool vec, float (&v)[NCH][8]) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = i * 512 + lane * 8;
    if (c < cols) {
      if (vec) load8f<T>(row + c, v[i]);
      else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = (c + e < cols) ? Elem<T>::to_f(row[c + e]) : 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
    }
  }
}
template <typename T, int NCH>
__device__ __forceinline__ void store_row(T* row, int cols, int lane, bool vec, const float (&v)[NCH][8]) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = i * 512 + lane * 8;
    if (c < cols) {
      if (vec) store8f<T>(row + c, v[i]);
      else {
#pragma unroll
        for (int e = 0; e < 8; ++e) if (c + e < cols) row[c + e] = Elem<T>::from_f(v[i][e]);
      }
    }
  }
}

template <typename T, int NCH>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, T* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd,
                                                     long long rows, int cols, float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bool vec = (cols % 8) == 0;
  float v[NCH][8];
  load_row<T, NCH>(x + row * cols, cols, lane, vec, v);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[i][e];
  const float mu = wave_sum(s) / (float)cols;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = i * 512 + lane * 8 + e;
      const float d = c < cols ? v[i][e] - mu : 0.f;
      q += d * d;
    }
  const float rs = rsqrtf(wave_sum(q) / (float)cols + eps);
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = i * 512 + lane * 8 + e;
      if (c < cols) v[i][e] = (v[i][e] - mu) * rs * gamma[c] + beta[c];
    }
  store_row<T, NCH>(y + row * cols, cols, lane, vec, v);
  if (lane == 0) { if (mean) mean[row] = mu; if (rstd) rstd[row] = rs; }
}

template <typename T, int NCH>
__global__ __launch_bounds__(256) void ln_bwd_dx_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, T* __restrict__ dx,
                                                        long long rows, int cols) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bool vec = (cols % 8) == 0;
  float xv[NCH][8], gv[NCH][8];
  load_row<T, NCH>(x + row * cols, cols, lane, vec, xv);
  load_row<T, NCH>(dy + row * cols, cols, lane, vec, gv);
  const float mu = mean[row], rs = rstd[row];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = i * 512 + lane * 8 + e;
      if (c < cols) {
        const float xh = (xv[i][e] - mu) * rs;
        const float g = gv[i][e] * gamma[c];
        xv[i][e] = xh; gv[i][e] = g;
        s1 += g; s2 += g * xh;
      }
    }
  s1 = wave_sum(s1) / (float)cols;
  s2 = wave_sum(s2) / (float)cols;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) gv[i][e] = rs * (gv[i][e] - s1 - xv[i][e] * s2);
  store_row<T, NCH>(dx + row * cols, cols, lane, vec, gv);
}


// ------------------------------------------------------------------------------------------------
// Vector (cols % 4 == 0) LayerNorm kernels.  Lane l owns the 4-element vectors l, l+64, ... of a row (NV per lane),
// so 768 columns split evenly over the wave (3 x 8-byte bf16 loads per lane and row, 512 contiguous bytes per wave
// instruction).  A wave works on RPW rows at a time with all their loads issued before the first reduction, and loads
// gamma/beta once.  Backward is one pass: dx plus per-lane dgamma/dbeta partial sums kept in registers across the
// wave's rows, reduced over the block through LDS into a [blocks][2][cols] workspace; a tiny second kernel folds the
// workspace into dgamma/dbeta (+=).
// ------------------------------------------------------------------------------------------------
constexpr int RPW = 4;          // rows per wave per iteration (forward)
constexpr int BRPW = 4;         // rows per wave and register set of the backward (two sets in flight)
int g_ln_max_blocks = 256;     // blocks of the single-pass LayerNorm backward (A/B: st5_layernorm_set_max_blocks)

template <typename T> __device__ __forceinline__ void load4f(const T* p, float (&v)[4]);
template <> __device__ __forceinline__ void load4f<float>(const float* p, float (&v)[4]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = a[i];
}
template <> __device__ __forceinline__ void load4f<bf16_t>(const bf16_t* p, float (&v)[4]) {
  const u32x2 a = *reinterpret_cast<const u32x2*>(p);
  v[0] = __uint_as_float(a[0] << 16); v[1] = __uint_as_float(a[0] & 0xffff0000u);
  v[2] = __uint_as_float(a[1] << 16); v[3] = __uint_as_float(a[1] & 0xffff0000u);
}
template <typename T> __device__ __forceinline__ void store4f(T* p, const float (&v)[4]);
template <> __device__ __forceinline__ void store4f<float>(float* p, const float (&v)[4]) {
  f32x4 a;
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = v[i];
  *reinterpret_cast<f32x4*>(p) = a;
}
template <> __device__ __forceinline__ void store4f<bf16_t>(bf16_t* p, const float (&v)[4]) {
  bf16x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (bf16_t)v[i];
  *reinterpret_cast<bf16x4*>(p) = o;
}

// Q8 (round 6, fp8 compute mode): the output row is ALSO written as its MX-fp8 image (q8: e4m3 bytes [rows x cols], s8: one e8m0 scale
// byte per 32 columns) -- the bytes st5_quant_mxfp8 produces from y, so the fp8 GEMMs that read a pre-LN layer's LayerNorm output (QKV,
// fc1: models/speecht5.py:1402-1425 `encoder_normalize_before`) need no quantisation pass.  A lane holds 4 consecutive columns, 8
// lanes one MX block (blocks start at multiples of 32 columns = 8 lanes).
// ACT (round 6; the layer-norm convolution extractor of t5_transformer_large, speech_encoder_prenet.py:318-331: LayerNorm + GELU behind every
// convolution): y = GELU(LN(x)) in one pass -- the composition ran a LayerNorm pass and an activation pass over 2 GB at B = 32.
template <typename T, int NV, bool Q8 = false, bool ACT = false>
__global__ __launch_bounds__(256) void ln_fwd_vec_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, T* __restrict__ y,
                                                         float* __restrict__ mean, float* __restrict__ rstd,
                                                         long long rows, int cols, float eps,
                                                         const float* __restrict__ keep, const T* __restrict__ skip,
                                                         unsigned char* __restrict__ q8 = nullptr, unsigned char* __restrict__ s8 = nullptr,
                                                         const float* __restrict__ gate = nullptr) {
  // gate (layer gate, st5_layernorm_fwd_gate): *gate == 0 -> a LayerNorm inside a dropped layer exits (y, mean, rstd are read by that
  // layer alone); the layer's LAST LayerNorm (skip given) writes y = skip without reading x, mean / rstd stay unwritten
  if (st5_gate_dropped(gate)) {
    if (skip == nullptr) return;
    const int lane_ = threadIdx.x & 63;
    const long long r0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      if (r0 + r >= rows) break;
      const long long ro = (r0 + r) * cols;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane_) * 4;
        if (c < cols) { float o[4]; load4f<T>(skip + ro + c, o); store4f<T>(y + ro + c, o); }
      }
    }
    return;
  }
  // keep / skip (LayerDrop gate, st5_layernorm_gated_fwd): *keep == 0 -> y = skip (the layer's input) instead of LN(x)
  const bool dropped = keep != nullptr && *keep == 0.f;
  const int lane = threadIdx.x & 63;
  const long long row0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
  if (row0 >= rows) return;
  float v[RPW][NV][4];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const long long row = row0 + r < rows ? row0 + r : rows - 1;
    long long ro = row * cols;             // (once per row, opaque: see ln_bwd_vec_kernel)
    asm volatile("" : "+v"(ro));
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < cols) load4f<T>(x + ro + c, v[r][i]);
      else { v[r][i][0] = v[r][i][1] = v[r][i][2] = v[r][i][3] = 0.f; }
    }
  }
  float g[NV][4], b[NV][4];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < cols) { load4f<float>(gamma + c, g[i]); load4f<float>(beta + c, b[i]); }
    else { g[i][0] = g[i][1] = g[i][2] = g[i][3] = 0.f; b[i][0] = b[i][1] = b[i][2] = b[i][3] = 0.f; }
  }
  const float inv_n = 1.f / (float)cols;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) s += v[r][i][e];
    const float mu = wave_sum(s) * inv_n;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const bool in = (i * 64 + lane) * 4 < cols;
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float d = in ? v[r][i][e] - mu : 0.f; v[r][i][e] = d; q += d * d; }
    }
    const float rs = rsqrtf(wave_sum(q) * inv_n + eps);
    if (row0 + r < rows) {
      long long ro = (row0 + r) * cols;
      asm volatile("" : "+v"(ro));
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < cols) {
          float o[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = fmaf(v[r][i][e] * rs, g[i][e], b[i][e]);
          if constexpr (ACT) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = act_f<sizeof(T) == 2>(ACT_GELU, o[e]);
          }
          if (dropped) load4f<T>(skip + ro + c, o);
          store4f<T>(y + ro + c, o);
          if constexpr (Q8) {
            // (cols % 32 == 0: the 8 lanes of a block are all inside the row or all outside)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = Elem<T>::to_f(Elem<T>::from_f(o[e]));        // the values the bf16 output holds
            unsigned int qw[1], qs;
            mx8_quant<4>(o, qw, qs);
            *reinterpret_cast<unsigned int*>(q8 + ro + c) = qw[0];
            if ((lane & 7) == 0) s8[(row0 + r) * (cols >> 5) + (c >> 5)] = (unsigned char)qs;
          }
        }
      }
      if (lane == 0) { if (mean) mean[row0 + r] = mu; if (rstd) rstd[row0 + r] = rs; }
    }
  }
}

// dx (+ block partials of dgamma/dbeta when PG).  part: [gridDim.x][2][cols]
// dxd (optional): second output dx * dropout_mask(seed, row * cols + c) -- the gradient the Linear in front of this
// LayerNorm needs when its output went through the fused dropout epilogue (y = residual + drop(x W^T + b); LN(y)),
// produced here instead of by a separate dropout kernel over dx.
// ACTB: the forward was y = GELU(LN(x)) (ln_fwd_vec_kernel<.., ACT>): the incoming gradient is multiplied by GELU'(z), z = LN(x) recomputed
// from x, mean, rstd, gamma and `beta` -- no pre-activation tensor is kept and no activation-backward pass runs.
template <typename T, int NV, bool PG, bool ACTB = false>
__global__ __launch_bounds__(256) void ln_bwd_vec_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                         const float* __restrict__ gamma, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, T* __restrict__ dx,
                                                         float* __restrict__ part, long long rows, int cols,
                                                         T* __restrict__ dxd, float drop_p, unsigned long long seed,
                                                         const float* __restrict__ keep, const float* __restrict__ beta = nullptr,
                                                         const T* __restrict__ addend = nullptr, const float* __restrict__ gate = nullptr) {
  // gate (layer gate, st5_layernorm_bwd_gate): *gate == 0 -> the LayerNorm belongs to a dropped layer: dy, x, mean and rstd are not read
  // (the skipped forward never wrote them), dx / dxd are not written (only that layer's launches would read them) and the block
  // partials are stored as zeros, so that the immediate or deferred final reduction adds nothing to dgamma / dbeta
  if (st5_gate_dropped(gate)) {
    if (PG)
      for (int c = threadIdx.x; c < 2 * cols; c += 256) part[(long long)blockIdx.x * 2 * cols + c] = 0.f;
    return;
  }
  // addend (st5_layernorm_bwd_add, round 6): dx = LayerNorm backward + addend -- the gradient of a pre-LN block's residual connection
  // (y = x + f(LN(x))), handed over by the Linear that added the residual, so that autograd does not sum the two with a kernel of its own
  // keep (LayerDrop gate, st5_layernorm_gated_bwd): *keep == 0 -> the incoming gradient counts as zero (dx = 0, no dgamma / dbeta)
  const bool dropped = keep != nullptr && *keep == 0.f;
  const unsigned int thresh = dxd ? dropout_thresh(drop_p) : 0u;
  const float inv_keep = dxd ? 1.f / (1.f - drop_p) : 1.f;
  const unsigned int seedf = dxd ? drop_seed_fold(seed) : 0u;      // (once: see dropout_scale4_folded)
  extern __shared__ float red[];   // PG: [4 waves][2][cols]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float g[NV][4], dg[NV][4], db[NV][4];
  float bb[ACTB ? NV : 1][4];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < cols) load4f<float>(gamma + c, g[i]);
    else { g[i][0] = g[i][1] = g[i][2] = g[i][3] = 0.f; }
    if constexpr (ACTB) {
      if (c < cols) load4f<float>(beta + c, bb[i]);
      else { bb[i][0] = bb[i][1] = bb[i][2] = bb[i][3] = 0.f; }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { dg[i][e] = 0.f; db[i][e] = 0.f; }
  }
  const float inv_n = 1.f / (float)cols;
  // Two register sets in ping-pong: the loads of the wave's NEXT rows are issued before the reductions and stores of the current
  // ones (a wave is alone on its SIMD here -- one block per CU -- so nothing else would cover the HBM latency of a trip).
  // (operands are kept as loaded -- 8 bytes per 4 bf16 -- and converted when used: two sets of BRPW rows fit in ~100 registers)
  struct alignas(sizeof(T) * 4) Raw4 { T v[4]; };
  struct Set { Raw4 xv[BRPW][NV], gv[BRPW][NV]; float mu[BRPW], rs[BRPW]; };
  auto load_set = [&](Set& S, long long row0) {
    // (row offsets: ONE 64-bit multiply per set, opaque, + r * cols on the scalar unit; hipcc otherwise forms row * cols + c as a 64-bit
    //  multiply-add -- a quarter-rate instruction -- per access: 120 of them per trip of this loop at 768 columns, on a kernel that runs
    //  one wave per SIMD)
    long long ro0 = row0 * cols;
    asm volatile("" : "+v"(ro0));
    const long long ro_last = (rows - 1) * cols;
#pragma unroll
    for (int r = 0; r < BRPW; ++r) {
      const long long row = row0 + r < rows ? row0 + r : rows - 1;
      long long ro = ro0 + (long long)r * cols;
      ro = ro < ro_last ? ro : ro_last;
      const T* const xr = x + ro;
      const T* const gr = dy + ro;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < cols) {
          S.xv[r][i] = *reinterpret_cast<const Raw4*>(xr + c);
          S.gv[r][i] = *reinterpret_cast<const Raw4*>(gr + c);
        }
      }
      S.mu[r] = mean[row]; S.rs[r] = rstd[row];
    }
  };
  auto finish_set = [&](Set& S, long long row0) {
    long long fo0 = row0 * cols;
    asm volatile("" : "+v"(fo0));
#pragma unroll
    for (int r = 0; r < BRPW; ++r) {
      const bool live = row0 + r < rows;
      float s1 = 0.f, s2 = 0.f;
      float xh_[NV][4], gg_[NV][4];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const bool in = (i * 64 + lane) * 4 < cols;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xh = in ? (Elem<T>::to_f(S.xv[r][i].v[e]) - S.mu[r]) * S.rs[r] : 0.f;
          float d = (in && !dropped) ? Elem<T>::to_f(S.gv[r][i].v[e]) : 0.f;
          if constexpr (ACTB) d *= act_grad_f<sizeof(T) == 2>(ACT_GELU, fmaf(xh, g[i][e], bb[i][e]));
          if (PG && live) { dg[i][e] = fmaf(d, xh, dg[i][e]); db[i][e] += d; }
          const float gg = d * g[i][e];
          xh_[i][e] = xh; gg_[i][e] = gg;
          s1 += gg; s2 = fmaf(gg, xh, s2);
        }
      }
      s1 = wave_sum(s1) * inv_n;
      s2 = wave_sum(s2) * inv_n;
      if (live) {
        const long long ro = fo0 + (long long)r * cols;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int c = (i * 64 + lane) * 4;
          if (c < cols) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = S.rs[r] * (gg_[i][e] - s1 - xh_[i][e] * s2);
            if (addend) {
              float a4[4];
              load4f<T>(addend + ro + c, a4);
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] += a4[e];
            }
            store4f<T>(dx + ro + c, o);
            if (dxd) {
              float dsc[4];
              dropout_scale4_folded(seedf, (unsigned long long)(ro + c), thresh, inv_keep, dsc);
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = Elem<T>::to_f(Elem<T>::from_f(o[e])) * dsc[e];  // mask the ROUNDED dX
              store4f<T>(dxd + ro + c, o);
            }
          }
        }
      }
    }
  };
  {
    const long long stride = (long long)gridDim.x * 4 * BRPW;
    long long row0 = ((long long)blockIdx.x * 4 + wave) * BRPW;
    Set A, B;
    if (row0 < rows) {
      load_set(A, row0);
      while (true) {
        const long long r1 = row0 + stride;
        if (r1 < rows) load_set(B, r1);
        finish_set(A, row0);
        if (r1 >= rows) break;
        const long long r2 = r1 + stride;
        if (r2 < rows) load_set(A, r2);
        finish_set(B, r1);
        if (r2 >= rows) break;
        row0 = r2;
      }
    }
  }
  if (PG) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < cols) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { red[(wave * 2 + 0) * cols + c + e] = dg[i][e]; red[(wave * 2 + 1) * cols + c + e] = db[i][e]; }
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * cols; c += 256)
      part[(long long)blockIdx.x * 2 * cols + c] = red[c] + red[2 * cols + c] + red[4 * cols + c] + red[6 * cols + c];
  }
}

// dgamma[c] += sum_b part[b][0][c];  dbeta[c] += sum_b part[b][1][c]   (block = 64 columns x 16 partial-row lanes)
__global__ __launch_bounds__(1024) void ln_bwd_final_kernel(const float* __restrict__ part, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int nblk, int cols) {
  __shared__ float red[16][64];
  const int cl = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;     // index into [2][cols]
  float s = 0.f;
  if (c < 2 * cols)
    for (int b = j; b < nblk; b += 16) s += part[(long long)b * 2 * cols + c];
  red[j][cl] = s;
  __syncthreads();
  if (j == 0 && c < 2 * cols) {
    s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[k][cl];
    if (c < cols) { if (dgamma) dgamma[c] += s; }
    else if (dbeta) dbeta[c - cols] += s;
  }
}

// Deferred form of the reduction above: while st5_layernorm_defer is on, every LayerNorm backward leaves its block partials
// in an arena slot and ONE launch per flush folds the partials of all pending LayerNorms into their dgamma / dbeta (the
// training step has ~86 LayerNorm backwards, each followed by a 7 us reduction launch).  Descriptors travel as a kernel
// argument; a block finds its descriptor by its block range.
constexpr int LNF_MAX = 48;
struct LnFinalDesc { const float* part; float* dgamma; float* dbeta; int nblk, cols, blk0, pad; };
struct LnFinalArgs { LnFinalDesc d[LNF_MAX]; int n; };
__global__ __launch_bounds__(1024) void ln_bwd_final_multi_kernel(const LnFinalArgs a) {
  __shared__ float red[16][64];
  int k = 0;
  while (k + 1 < a.n && (int)blockIdx.x >= a.d[k + 1].blk0) ++k;
  const LnFinalDesc d = a.d[k];
  const int cl = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int c = ((int)blockIdx.x - d.blk0) * 64 + cl;     // index into [2][cols]
  float s = 0.f;
  if (c < 2 * d.cols)
    for (int b = j; b < d.nblk; b += 16) s += d.part[(long long)b * 2 * d.cols + c];
  red[j][cl] = s;
  __syncthreads();
  if (j == 0 && c < 2 * d.cols) {
    s = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += red[q][cl];
    if (c < d.cols) { if (d.dgamma) d.dgamma[c] += s; }
    else if (d.dbeta) d.dbeta[c - d.cols] += s;
  }
}
bool g_ln_defer = false;
// deferred-reduction state, one per stream and never handed to another (stream_scratch.h; as the split-K states of gemm.hip: two
// backward passes may run on two streams, and the second must not write its partials into the arena the first one's queued
// reduction still has to read)
struct LnDeferState {
  LnFinalArgs pending = {};
  int blocks = 0;
  BumpArena<St5Dev> arena;   // block partials of the queued reductions
  // folds everything queued into its dgamma / dbeta with one launch on the state's stream
  int flush(hipStream_t stream) {
    if (pending.n == 0) return ST5_OK;
    hipLaunchKernelGGL(ln_bwd_final_multi_kernel, dim3((unsigned)blocks), dim3(1024), 0, stream, pending);
    pending.n = 0; blocks = 0; arena.reset();
    HIP_CHECK_LAUNCH();
    return ST5_OK;
  }
};
PerStream<LnDeferState> g_lnstates;
int ln_flush(hipStream_t s) {
  LnDeferState* ls = g_lnstates.find(s);
  return ls ? ls->flush(s) : (int)ST5_OK;
}

int ln_blocks(long long rows) {
  long long n = (rows + 4 * BRPW - 1) / (4 * BRPW);   // blocks at one trip per wave
  if (n < 1) n = 1;
  if (n <= g_ln_max_blocks) return (int)n;
  const long long trips = (n + g_ln_max_blocks - 1) / g_ln_max_blocks;   // same number of trips for every wave
  return (int)((n + trips - 1) / trips);
}

// ---- column reductions: out[c] (+)= scale * sum_r f(r, c) --------------------------------------
// MODE 0: f = x            MODE 1: f = dy * (x - mean[r]) * rstd[r]   (LayerNorm dgamma)
// Stage 1: grid (ceil(cols/256), nsplit), 256 threads = 32 column-groups(8 cols) x 8 row lanes.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void colreduce_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                        const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, float* __restrict__ part,
                                                        long long rows, int cols, long long ld, const float* __restrict__ gate = nullptr) {
  if (st5_gate_dropped(gate)) return;    // (colreduce_final_kernel then writes zeros without reading the partials)
  __shared__ float red[8][256 + 8];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = blockIdx.x * 256 + tx * 8;
  const bool vec = (ld % 8) == 0 && c0 + 8 <= cols;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (c0 < cols) {
    for (long long r = (long long)blockIdx.y * 8 + ty; r < rows; r += (long long)gridDim.y * 8) {
      float a[8], b[8];
      if (vec) load8f<T>(x + r * ld + c0, a);
      else {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = (c0 + e < cols) ? Elem<T>::to_f(x[r * ld + c0 + e]) : 0.f;
      }
      if (MODE == 1) {
        if (vec) load8f<T>(dy + r * ld + c0, b);
        else {
#pragma unroll
          for (int e = 0; e < 8; ++e) b[e] = (c0 + e < cols) ? Elem<T>::to_f(dy[r * ld + c0 + e]) : 0.f;
        }
        const float mu = mean[r], rs = rstd[r];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += b[e] * (a[e] - mu) * rs;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += a[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[ty][tx * 8 + e] = acc[e];
  __syncthreads();
  const int c = threadIdx.x;
  if (blockIdx.x * 256 + c < cols) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += red[j][c];
    part[(long long)blockIdx.y * cols + blockIdx.x * 256 + c] = s;
  }
}
__global__ void colreduce_final_kernel(const float* __restrict__ part, float* __restrict__ out, int nsplit, int cols,
                                       float scale, int accumulate, const float* __restrict__ gate = nullptr) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  if (st5_gate_dropped(gate)) {          // a dropped layer's column sum is LIVE (its dPE gradient): exact zeros / an unchanged accumulator
    if (!accumulate) out[c] = 0.f;
    return;
  }
  float s = 0.f;
  for (int j = 0; j < nsplit; ++j) s += part[(long long)j * cols + c];
  s *= scale;
  out[c] = accumulate ? out[c] + s : s;
}

int nsplit_for(long long rows) {
  long long n = (rows + 63) / 64;
  if (n < 1) n = 1;
  if (n > 64) n = 64;
  return (int)n;
}

template <typename T, int MODE>
int colreduce(const void* x, const void* dy, const float* mean, const float* rstd, float* out, float* ws,
              long long rows, int cols, long long ld, float scale, int accumulate, hipStream_t s, const float* gate = nullptr) {
  const int ns = nsplit_for(rows);
  dim3 grid((cols + 255) / 256, ns);
  // two stages in both forms (block partials -> ordered final sum; `accumulate` adds to out[] there): the single-launch
  // variant with fp32 atomics made bias gradients depend on the order in which blocks retire
  hipLaunchKernelGGL((colreduce_kernel<T, MODE>), grid, dim3(256), 0, s, (const T*)x, (const T*)dy, mean, rstd, ws,
                     rows, cols, ld, gate);
  hipLaunchKernelGGL(colreduce_final_kernel, dim3((cols + 255) / 256), dim3(256), 0, s, ws, out, ns, cols, scale,
                     accumulate, gate);
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}

}  // namespace

static int layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean,
                         float* rstd, int64_t rows, int32_t cols, float eps, int dtype, void* stream, const float* keep, const void* skip,
                         const float* gate = nullptr) {
  if (!x || !y || !gamma || !beta || rows < 0 || cols <= 0 || cols > MAXCH * 512) return ST5_ERR_ARG;
  if (keep && (!skip || cols % 4 != 0 || cols > 2048)) return ST5_ERR_ARG;    // (the gate lives in the vector kernels only)
  if (gate && ((skip && !keep) || cols % 4 != 0 || cols > 2048)) return ST5_ERR_ARG;   // (and so does the layer gate: no ungated fall-back)
  if (rows == 0) return ST5_OK;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype != ST5_BF16 && dtype != ST5_F32) return ST5_ERR_ARG;
  if (cols % 4 == 0 && cols <= 2048) {   // vector kernels (every width of the model)
    dim3 vgrid((unsigned)((rows + 4 * RPW - 1) / (4 * RPW)));
#define LNV(TT, NV_)                                                                                                 \
  hipLaunchKernelGGL((ln_fwd_vec_kernel<TT, NV_>), vgrid, dim3(256), 0, s, (const TT*)x, gamma, beta, (TT*)y, mean, rstd, \
                     (long long)rows, cols, eps, keep, (const TT*)skip, (unsigned char*)nullptr, (unsigned char*)nullptr, gate)
#define LNV_T(TT)                                                                                                     \
  do {                                                                                                                \
    if (cols <= 256) LNV(TT, 1); else if (cols <= 512) LNV(TT, 2); else if (cols <= 768) LNV(TT, 3);                  \
    else if (cols <= 1024) LNV(TT, 4); else if (cols <= 1536) LNV(TT, 6); else LNV(TT, 8);                            \
  } while (0)
    if (dtype == ST5_BF16) LNV_T(bf16_t); else LNV_T(float);
#undef LNV_T
#undef LNV
    HIP_CHECK_LAUNCH();
    return ST5_OK;
  }
#define LNF(TT, NCH)                                                                                              \
  hipLaunchKernelGGL((ln_fwd_kernel<TT, NCH>), grid, dim3(256), 0, s, (const TT*)x, gamma, beta, (TT*)y, mean, rstd, \
                     (long long)rows, cols, eps)
#define LNF_T(TT)                                                                                \
  do {                                                                                           \
    if (cols <= 512) LNF(TT, 1); else if (cols <= 1024) LNF(TT, 2); else if (cols <= 2048) LNF(TT, 4); else LNF(TT, 8); \
  } while (0)
  if (dtype == ST5_BF16) LNF_T(bf16_t); else LNF_T(float);
#undef LNF_T
#undef LNF
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}

extern "C" int st5_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean,
                                 float* rstd, int64_t rows, int32_t cols, float eps, int dtype, void* stream) {
  return layernorm_fwd(x, gamma, beta, y, mean, rstd, rows, cols, eps, dtype, stream, nullptr, nullptr);
}
/* st5_layernorm_fwd (bf16, cols % 32 == 0, cols <= 2048) that also writes y's MX-fp8 image: q [rows x cols] e4m3 bytes, s [rows x cols/32]
 * e8m0 scale bytes -- what st5_quant_mxfp8 would produce from y.  fp8 compute mode, pre-LN layers (t5_transformer_large). */
extern "C" int st5_layernorm_fwd_q8(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, void* q, uint8_t* sc,
                                    int64_t rows, int32_t cols, float eps, void* stream) {
  if (!x || !y || !gamma || !beta || !q || !sc || rows < 0 || cols <= 0 || cols % 32 || cols > 2048) return ST5_ERR_ARG;
  if (rows == 0) return ST5_OK;
  hipStream_t s = (hipStream_t)stream;
  dim3 vgrid((unsigned)((rows + 4 * RPW - 1) / (4 * RPW)));
#define LNQ(NV_)                                                                                                                       \
  hipLaunchKernelGGL((ln_fwd_vec_kernel<bf16_t, NV_, true>), vgrid, dim3(256), 0, s, (const bf16_t*)x, gamma, beta, (bf16_t*)y, mean, rstd, \
                     (long long)rows, cols, eps, (const float*)nullptr, (const bf16_t*)nullptr, (unsigned char*)q, (unsigned char*)sc)
  if (cols <= 256) LNQ(1); else if (cols <= 512) LNQ(2); else if (cols <= 768) LNQ(3);
  else if (cols <= 1024) LNQ(4); else if (cols <= 1536) LNQ(6); else LNQ(8);
#undef LNQ
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}
/* y = GELU(LN(x) * gamma + beta) in one pass (cols % 4 == 0, cols <= 512: the layer-norm convolution extractor of t5_transformer_large,
 * speech_encoder_prenet.py:318-331); mean / rstd as st5_layernorm_fwd.  The bf16 form uses the GELU polynomial of the GEMM epilogues. */
extern "C" int st5_layernorm_gelu_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                      int64_t rows, int32_t cols, float eps, int dtype, void* stream) {
  if (!x || !y || !gamma || !beta || rows < 0 || cols <= 0 || cols % 4 || cols > 512) return ST5_ERR_ARG;
  if (dtype != ST5_BF16 && dtype != ST5_F32) return ST5_ERR_ARG;
  if (rows == 0) return ST5_OK;
  hipStream_t s = (hipStream_t)stream;
  dim3 vgrid((unsigned)((rows + 4 * RPW - 1) / (4 * RPW)));
#define LNA(TT, NV_)                                                                                                                      \
  hipLaunchKernelGGL((ln_fwd_vec_kernel<TT, NV_, false, true>), vgrid, dim3(256), 0, s, (const TT*)x, gamma, beta, (TT*)y, mean, rstd,    \
                     (long long)rows, cols, eps, (const float*)nullptr, (const TT*)nullptr, (unsigned char*)nullptr, (unsigned char*)nullptr)
  if (dtype == ST5_BF16) { if (cols <= 256) LNA(bf16_t, 1); else LNA(bf16_t, 2); }
  else { if (cols <= 256) LNA(float, 1); else LNA(float, 2); }
#undef LNA
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}
/* Backward of st5_layernorm_gelu_fwd: dx (and dgamma / dbeta accumulated, ws as st5_layernorm_bwd_ws_bytes says) from the gradient of
 * the ACTIVATED output; the pre-activation LN(x) is recomputed from x, mean, rstd, gamma, beta. */
extern "C" int st5_layernorm_gelu_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                      void* dx, float* dgamma, float* dbeta, void* ws, int64_t rows, int32_t cols, int dtype, void* stream) {
  if (!dy || !x || !gamma || !beta || !mean || !rstd || !dx || rows < 0 || cols <= 0 || cols % 4 || cols > 512) return ST5_ERR_ARG;
  if ((dgamma || dbeta) && !ws) return ST5_ERR_ARG;
  if (dtype != ST5_BF16 && dtype != ST5_F32) return ST5_ERR_ARG;
  if (rows == 0) return ST5_OK;
  hipStream_t s = (hipStream_t)stream;
  const int nb = ln_blocks(rows);
  const bool pg = dgamma || dbeta;
  const size_t shm = pg ? (size_t)8 * cols * sizeof(float) : 0;
#define LBA(TT, NV_)                                                                                                                       \
  do {                                                                                                                                     \
    if (pg) hipLaunchKernelGGL((ln_bwd_vec_kernel<TT, NV_, true, true>), dim3(nb), dim3(256), shm, s, (const TT*)dy, (const TT*)x, gamma,  \
                               mean, rstd, (TT*)dx, (float*)ws, (long long)rows, cols, (TT*)nullptr, 0.f, 0ull, (const float*)nullptr, beta); \
    else hipLaunchKernelGGL((ln_bwd_vec_kernel<TT, NV_, false, true>), dim3(nb), dim3(256), 0, s, (const TT*)dy, (const TT*)x, gamma,      \
                            mean, rstd, (TT*)dx, (float*)ws, (long long)rows, cols, (TT*)nullptr, 0.f, 0ull, (const float*)nullptr, beta); \
  } while (0)
  if (dtype == ST5_BF16) { if (cols <= 256) LBA(bf16_t, 1); else LBA(bf16_t, 2); }
  else { if (cols <= 256) LBA(float, 1); else LBA(float, 2); }
#undef LBA
  if (pg) hipLaunchKernelGGL(ln_bwd_final_kernel, dim3((2 * cols + 63) / 64), dim3(1024), 0, s, (const float*)ws, dgamma, dbeta, nb, cols);
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}
extern "C" int st5_layernorm_gated_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                       int64_t rows, int32_t cols, float eps, const float* keep, const void* skip, int dtype, void* stream) {
  if (!keep || !skip) return ST5_ERR_ARG;
  return layernorm_fwd(x, gamma, beta, y, mean, rstd, rows, cols, eps, dtype, stream, keep, skip);
}
/* st5_layernorm_fwd (keep == skip == NULL) or st5_layernorm_gated_fwd (both given) carrying the layer gate: *gate == 0 -> a plain LayerNorm
 * writes nothing, a gated one writes y = skip without reading x and leaves mean / rstd alone.  gate NULL or *gate != 0: the ungated call. */
extern "C" int st5_layernorm_fwd_gate(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int64_t rows,
                                      int32_t cols, float eps, const float* keep, const void* skip, const float* gate, int dtype,
                                      void* stream) {
  if ((keep == nullptr) != (skip == nullptr)) return ST5_ERR_ARG;
  return layernorm_fwd(x, gamma, beta, y, mean, rstd, rows, cols, eps, dtype, stream, keep, skip, gate);
}

extern "C" int64_t st5_layernorm_bwd_ws_bytes(int64_t rows, int32_t cols) {
  const int64_t a = (int64_t)nsplit_for(rows) * cols * sizeof(float);
  const int64_t b = (int64_t)ln_blocks(rows) * 2 * cols * sizeof(float);
  return a > b ? a : b;
}

static int layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean,
                         const float* rstd, void* dx, float* dgamma, float* dbeta, void* ws, int64_t rows,
                         int32_t cols, void* dx_dropped, float drop_p, uint64_t drop_seed, int dtype, void* stream, const float* keep,
                         const void* addend = nullptr, const float* gate = nullptr) {
  if (addend && (!dx || cols % 4 || cols > 2048)) return ST5_ERR_ARG;
  if (gate && (!dx || cols % 4 || cols > 2048)) return ST5_ERR_ARG;      // (the layer gate lives in the vector kernel only)
  if (keep && (!dx || cols % 4 || cols > 2048)) return ST5_ERR_ARG;
  if (dx_dropped && (!dx || cols % 4 || cols > 2048 || drop_p <= 0.f || drop_p >= 1.f)) return ST5_ERR_ARG;
  if (!dy || !x || !gamma || !mean || !rstd || rows < 0 || cols <= 0 || cols > MAXCH * 512) return ST5_ERR_ARG;
  if ((dgamma || dbeta) && !ws) return ST5_ERR_ARG;
  if (rows == 0) return ST5_OK;
  hipStream_t s = (hipStream_t)stream;
  if (dtype != ST5_BF16 && dtype != ST5_F32) return ST5_ERR_ARG;
  if (dx && cols % 4 == 0 && cols <= 2048) {   // single-pass vector path
    const int nb = ln_blocks(rows);
    const bool pg = dgamma || dbeta;
    const size_t shm = pg ? (size_t)8 * cols * sizeof(float) : 0;
    bool deferred = false;
    if (pg && g_ln_defer) {
      LnDeferState* ls = g_lnstates.get(s);
      // the same parameter twice in one batch (two micro-batches) would race inside the batched reduction: fold first
      for (int j = 0; j < ls->pending.n; ++j)
        if ((dgamma && ls->pending.d[j].dgamma == dgamma) || (dbeta && ls->pending.d[j].dbeta == dbeta)) {
          const int rc = ls->flush(s); if (rc) return rc; break;
        }
      if (ls->pending.n == LNF_MAX) { const int rc = ls->flush(s); if (rc) return rc; }
      // a full arena is emptied by a flush first and grown (outside capture only) when it is too small altogether
      const size_t need = (size_t)nb * 2 * cols * sizeof(float);
      ws = ls->arena.take(need);
      if (!ws) {
        const int rc = ls->flush(s); if (rc) return rc;
        if (!ls->arena.reserve(need, size_t(128) << 20, s)) return ST5_ERR_LAUNCH;
        ws = ls->arena.take(need);
      }
      LnFinalDesc& d = ls->pending.d[ls->pending.n++];
      d.part = reinterpret_cast<const float*>(ws); d.dgamma = dgamma; d.dbeta = dbeta; d.nblk = nb; d.cols = cols;
      d.blk0 = ls->blocks; d.pad = 0;
      ls->blocks += (2 * cols + 63) / 64;
      deferred = true;
    }
#define LBV(TT, NV_)                                                                                                    \
  do {                                                                                                                  \
    if (pg) hipLaunchKernelGGL((ln_bwd_vec_kernel<TT, NV_, true>), dim3(nb), dim3(256), shm, s, (const TT*)dy, (const TT*)x, gamma, \
                               mean, rstd, (TT*)dx, (float*)ws, (long long)rows, cols, (TT*)dx_dropped, drop_p,          \
                               (unsigned long long)drop_seed, keep, (const float*)nullptr, (const TT*)addend, gate);    \
    else hipLaunchKernelGGL((ln_bwd_vec_kernel<TT, NV_, false>), dim3(nb), dim3(256), 0, s, (const TT*)dy, (const TT*)x, gamma, \
                            mean, rstd, (TT*)dx, (float*)ws, (long long)rows, cols, (TT*)dx_dropped, drop_p,            \
                            (unsigned long long)drop_seed, keep, (const float*)nullptr, (const TT*)addend, gate);       \
  } while (0)
#define LBV_T(TT)                                                                                                     \
  do {                                                                                                                \
    if (cols <= 256) LBV(TT, 1); else if (cols <= 512) LBV(TT, 2); else if (cols <= 768) LBV(TT, 3);                  \
    else if (cols <= 1024) LBV(TT, 4); else if (cols <= 1536) LBV(TT, 6); else LBV(TT, 8);                            \
  } while (0)
    if (dtype == ST5_BF16) LBV_T(bf16_t); else LBV_T(float);
#undef LBV_T
#undef LBV
    if (pg && !deferred) hipLaunchKernelGGL(ln_bwd_final_kernel, dim3((2 * cols + 63) / 64), dim3(1024), 0, s, (const float*)ws, dgamma, dbeta, nb, cols);
    HIP_CHECK_LAUNCH();
    return ST5_OK;
  }
  // parameter gradients first (dx may alias dy)
  int rc = ST5_OK;
  if (dtype == ST5_BF16) {
    if (dgamma) rc |= colreduce<bf16_t, 1>(x, dy, mean, rstd, dgamma, (float*)ws, rows, cols, cols, 1.f, 1, s);
    if (dbeta) rc |= colreduce<bf16_t, 0>(dy, nullptr, nullptr, nullptr, dbeta, (float*)ws, rows, cols, cols, 1.f, 1, s);
  } else if (dtype == ST5_F32) {
    if (dgamma) rc |= colreduce<float, 1>(x, dy, mean, rstd, dgamma, (float*)ws, rows, cols, cols, 1.f, 1, s);
    if (dbeta) rc |= colreduce<float, 0>(dy, nullptr, nullptr, nullptr, dbeta, (float*)ws, rows, cols, cols, 1.f, 1, s);
  } else return ST5_ERR_ARG;
  if (rc) return rc;
  if (dx) {
    dim3 grid((unsigned)((rows + 3) / 4));
#define LNB(TT, NCH)                                                                                         \
  hipLaunchKernelGGL((ln_bwd_dx_kernel<TT, NCH>), grid, dim3(256), 0, s, (const TT*)dy, (const TT*)x, gamma, mean, \
                     rstd, (TT*)dx, (long long)rows, cols)
#define LNB_T(TT)                                                                                \
  do {                                                                                           \
    if (cols <= 512) LNB(TT, 1); else if (cols <= 1024) LNB(TT, 2); else if (cols <= 2048) LNB(TT, 4); else LNB(TT, 8); \
  } while (0)
    if (dtype == ST5_BF16) LNB_T(bf16_t); else LNB_T(float);
#undef LNB_T
#undef LNB
    HIP_CHECK_LAUNCH();
  }
  return ST5_OK;
}

extern "C" int st5_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean,
                                 const float* rstd, void* dx, float* dgamma, float* dbeta, void* ws, int64_t rows,
                                 int32_t cols, void* dx_dropped, float drop_p, uint64_t drop_seed, int dtype, void* stream) {
  return layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, rows, cols, dx_dropped, drop_p, drop_seed, dtype, stream, nullptr);
}
/* st5_layernorm_bwd with dx = (LayerNorm backward) + addend (same shape and dtype as dx; cols % 4 == 0, cols <= 2048): the residual gradient of a
 * pre-LN block folded into the LayerNorm backward at the block's input. */
extern "C" int st5_layernorm_bwd_add(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                                     float* dgamma, float* dbeta, void* ws, int64_t rows, int32_t cols, const void* addend, int dtype, void* stream) {
  if (!addend) return ST5_ERR_ARG;
  return layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, rows, cols, nullptr, 0.f, 0, dtype, stream, nullptr, addend);
}
extern "C" int st5_layernorm_gated_bwd(const void* dy, const void* x, const float* gamma, const float* mean,
                                       const float* rstd, void* dx, float* dgamma, float* dbeta, void* ws, int64_t rows,
                                       int32_t cols, void* dx_dropped, float drop_p, uint64_t drop_seed, const float* keep, int dtype,
                                       void* stream) {
  if (!keep) return ST5_ERR_ARG;
  return layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, rows, cols, dx_dropped, drop_p, drop_seed, dtype, stream, keep);
}
/* st5_layernorm_bwd (keep NULL) or st5_layernorm_gated_bwd carrying the layer gate: *gate == 0 -> no operand is read, dx / dx_dropped are not
 * written and nothing is added to dgamma / dbeta, with the immediate and with the deferred reduction (the block partials are zeros). */
extern "C" int st5_layernorm_bwd_gate(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                                      float* dgamma, float* dbeta, void* ws, int64_t rows, int32_t cols, void* dx_dropped, float drop_p,
                                      uint64_t drop_seed, const float* keep, const float* gate, int dtype, void* stream) {
  return layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, rows, cols, dx_dropped, drop_p, drop_seed, dtype, stream, keep,
                       nullptr, gate);
}

/* Deferred dgamma / dbeta reductions (see ln_bwd_final_multi_kernel).  While enabled, the parameter gradients of
 * st5_layernorm_bwd (vector path) are complete only after st5_layernorm_flush() on the same stream; disabling flushes. */
extern "C" int st5_layernorm_defer(int enabled, void* stream) {
  (void)stream;
  if (!enabled && g_ln_defer) {   // fold whatever is queued, every state on its own stream
    int rc = ST5_OK;
    g_lnstates.for_each([&rc](void* s, LnDeferState& ls) { if (!rc) rc = ls.flush(static_cast<hipStream_t>(s)); });
    if (rc) return rc;
  }
  g_ln_defer = enabled != 0;
  return ST5_OK;
}
extern "C" int st5_layernorm_flush(void* stream) { return ln_flush(reinterpret_cast<hipStream_t>(stream)); }
/* A/B switch: upper bound of the backward's block count (partials workspace = blocks x 2 x cols floats). */
extern "C" int st5_layernorm_set_max_blocks(int n) { if (n < 1 || n > 4096) return ST5_ERR_ARG; g_ln_max_blocks = n; return ST5_OK; }

// out[c] (+)= scale * sum_r x[r, c], in two stages through the caller's `ws` (hip.workspace: a per-stream buffer of the host side)
extern "C" int st5_colsum_ws(const void* x, float* out, void* ws, int64_t rows, int32_t cols, int64_t ld, float scale,
                             int32_t accumulate, int dtype, void* stream) {
  if (!x || !out || !ws || rows < 0 || cols <= 0) return ST5_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == ST5_BF16)
    return colreduce<bf16_t, 0>(x, nullptr, nullptr, nullptr, out, (float*)ws, rows, cols, ld, scale, accumulate, s);
  if (dtype == ST5_F32)
    return colreduce<float, 0>(x, nullptr, nullptr, nullptr, out, (float*)ws, rows, cols, ld, scale, accumulate, s);
  return ST5_ERR_ARG;
}
/* st5_colsum_ws carrying the layer gate: *gate == 0 -> x and the partials are not read; out = exact zeros (overwrite form) or unchanged. */
extern "C" int st5_colsum_ws_gate(const void* x, float* out, void* ws, int64_t rows, int32_t cols, int64_t ld, float scale,
                                  int32_t accumulate, const float* gate, int dtype, void* stream) {
  if (!x || !out || !ws || rows < 0 || cols <= 0) return ST5_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == ST5_BF16)
    return colreduce<bf16_t, 0>(x, nullptr, nullptr, nullptr, out, (float*)ws, rows, cols, ld, scale, accumulate, s, gate);
  if (dtype == ST5_F32)
    return colreduce<float, 0>(x, nullptr, nullptr, nullptr, out, (float*)ws, rows, cols, ld, scale, accumulate, s, gate);
  return ST5_ERR_ARG;
}
extern "C" int64_t st5_colsum_ws_bytes(int64_t rows, int32_t cols) {
  return (int64_t)nsplit_for(rows) * cols * sizeof(float);
}
