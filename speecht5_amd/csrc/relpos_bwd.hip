// Relative-position part of the encoder self-attention backward, behind the fused dq / dkv kernels.
//
// The dkv kernel leaves the bucket gradients dQP [B*H, T, nb] (bf16).  Two products fold them into the gradients:
//   dQ[bh][t][:]   += alpha * sum_b dQP[bh][t][b] * PE[b][:]          (M = T, N = 64, K = nb)
//   part[bh][b][:]  = alpha * sum_t dQP[bh][t][b] * Q[bh][t][:]       (M = nb, N = 64, K = T; fp32, summed over bh afterwards)
// st5_relpos_bwd does both in ONE launch that reads every dQP row once: one workgroup per (batch, head) walks the 64-query tiles
// in ascending order, holds the nb x 64 fp32 partial in accumulator registers for the whole walk and finishes each 64-query dQ tile
// as it passes.  st5_relpos_dpe_final is the ordered sum of the partials over (batch, head) and the cast, in one launch.
//
// Bits.  Both products are v_mfma_f32_32x32x16_bf16 chains over the reduction index in ascending chunks of 16, from zero, with the
// operand roles (A = the dQP side, B = PE / Q) and the k-to-lane map of the library's NT / TN GEMM kernels, and the epilogue
// arithmetic of gemm.hip's epilogue_fast (alpha * acc rounded, then + old dQ rounded, then the bf16 conversion): the results are
// the bytes st5_gemm produces for the same operands.  The final sum reproduces colreduce_kernel<float, 0> / colreduce_final_kernel
// of norm.hip term by term.
//
// LDS.  A tile of 64 dQP rows lives in ceil(nb / 128) panels of [64 rows][256 B] and the 64 Q rows in one more panel, copied
// HBM -> LDS by LDS-DMA, two tiles deep.  The 16-byte chunk ch of row r sits at 256 r + 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))):
// ONE image serves the row reads (ds_read_b128: dQP as the K-major A operand of the dQ product) and the transposed reads
// (ds_read_b64_tr_b16: dQP^T and Q^T as the operands of the dPE product) without bank conflicts.  PE, the B operand of the dQ
// product, is needed transposed as well; it is the same 40 KB for every tile, so each wave keeps its 32-column share as MFMA
// fragments in registers (80 VGPRs at nb = 320) for the whole walk, read once through the same image.
#include "common.h"
#include "../../include/speecht5_hip.h"

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;
typedef __attribute__((ext_vector_type(4))) short s16x4;

constexpr int RP_TQ = 64;            // queries per tile
constexpr int RP_PANEL = 64 * 256;   // one LDS panel: [64 rows][256 B]
constexpr int RP_ST_LD = 36;         // floats per staged dQ row (32 + 4 pad)
constexpr int RP_STAGE = 4 * 32 * RP_ST_LD * 4;

// rows past T and chunks past nb / past Q's 64 columns are copied from here: exact zeros in the sums, no read out of bounds
__device__ __attribute__((aligned(256))) char g_rp_zero[256];

__device__ __forceinline__ bf16x8 rp_tr_frag(const unsigned a0, const unsigned a1) {
  s16x4 lo, hi;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(a0) : "memory");
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(hi) : "v"(a1) : "memory");
  union { struct { s16x4 a, b; } s; bf16x8 v; } u;
  u.s.a = lo; u.s.b = hi;
  return u.v;
}
__device__ __forceinline__ bf16x8 rp_row_frag(const unsigned a) {
  bf16x8 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(a) : "memory");
  return v;
}
template <int N>
__device__ __forceinline__ void rp_lgkm_wait() { asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(N) : "memory"); }
__device__ __forceinline__ void rp_tie(bf16x8& f) { asm volatile("" : "+v"(f)); }

// NB64 = nb / 64.  256 threads = 4 waves, one per SIMD: wave w owns the 32 x 32 dQ tile (rows 32 (w >> 1), columns 32 (w & 1)) of every
// query tile and the NB64 32 x 32 tiles (bucket rows 32 ((w >> 1) + 2 i), columns 32 (w & 1)) of the dPE partial.
template <int NB64>
__global__ __launch_bounds__(256) void relpos_bwd_kernel(const bf16_t* __restrict__ dqp, const bf16_t* __restrict__ q, const long long q_ld,
                                                         const bf16_t* __restrict__ pe, bf16_t* __restrict__ dq, const long long dq_ld,
                                                         float* __restrict__ part, const int H, const int T, const float alpha,
                                                         const float* __restrict__ gate) {
  // (alpha * acc and the + old dQ are two roundings, as in the GEMM epilogue this kernel replaces)
#pragma clang fp contract(off)
  if (st5_gate_dropped(gate)) return;
  constexpr int NB = NB64 * 64;
  constexpr int NPAN = (NB64 + 1) / 2;
  constexpr int BUF = (NPAN + 1) * RP_PANEL;
  constexpr int NCH = NB / 16;           // k-chunks of the dQ product
  extern __shared__ __attribute__((aligned(256))) char dsm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int bh = blockIdx.x, bb = bh / H, hh = bh - bb * H;
  const bf16_t* const dqp_z = dqp + (long long)bh * T * NB;
  const bf16_t* const q_z = q + (long long)bb * T * q_ld + hh * 64;
  bf16_t* const dq_z = dq + (long long)bb * T * dq_ld + hh * 64;
  const bool want_part = part != nullptr;
  const int ntiles = (T + RP_TQ - 1) / RP_TQ;

  // ---- LDS-DMA sources.  A wave instruction fills 1 KB = 4 rows of a panel; wave w takes the 4-row slabs w, w + 4, ... of the tile's
  // (NPAN + 1) * 16.  Slab w + 4 i: panel i >> 2, rows 4 (w + 4 (i & 3)) + (lane >> 4); lane's physical chunk lane & 15 holds the logical
  // chunk below (row & 3 == lane >> 4 and (row >> 2) & 3 == w for every slab of this wave).
  const int lrow = lane >> 4;
  const int lch = (lane & 15) ^ ((lrow << 2) | wave);
  const bf16_t* const zero = reinterpret_cast<const bf16_t*>(g_rp_zero) + (lane & 15) * 8;
  auto issue = [&](const int tile, const int buf) {
    char* const base = dsm + buf * BUF + wave * 1024;
    const int t0 = tile * RP_TQ;
#pragma unroll
    for (int i = 0; i < NPAN * 4; ++i) {
      const int pan = i >> 2;
      const int t = t0 + (wave + 4 * (i & 3)) * 4 + lrow;
      const int col = pan * 128 + lch * 8;
      const bf16_t* src = (t < T && col < NB) ? dqp_z + (long long)t * NB + col : zero;
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(base + pan * RP_PANEL + (i & 3) * 4096), 16, 0, 0);
    }
    if (want_part) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = t0 + (wave + 4 * i) * 4 + lrow;
        const bf16_t* src = (t < T && lch < 8) ? q_z + (long long)t * q_ld + lch * 8 : zero;
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(base + NPAN * RP_PANEL + i * 4096), 16, 0, 0);
      }
    }
  };
  issue(0, 0);

  // ---- fragment addresses inside a tile buffer
  const unsigned lds_base = (unsigned)(size_t)(lds_ptr_t)dsm;
  // transposed reads: 16-lane group gi covers columns 16 (gi & 1) .. + 15 of the 32-column block and k rows 8 (gi >> 1) + q4 (+ 4 for the
  // second read); lane 4 q4 + p4 of the group supplies row q4's chunk (p4 >> 1), half (p4 & 1).  Row r = 16 kg + 8 kh2 + q4 + 4 rd: r & 3 = q4,
  // (r >> 2) & 3 = 2 kh2 + rd.
  const int gi = lane >> 4, mh = gi & 1, kh2 = gi >> 1, q4 = (lane & 15) >> 2, p4 = lane & 3;
  auto tr_off = [&](const int col32, const int rd) {    // col32: first column of the 32-column block inside its panel
    const int ch = (col32 >> 3) + 2 * mh + (p4 >> 1);
    const int r = 8 * kh2 + q4 + 4 * rd;
    return 256 * r + 16 * (ch ^ ((q4 << 2) | (2 * kh2 + rd))) + 8 * (p4 & 1);
  };
  unsigned ta[NB64][2], tb[2];
#pragma unroll
  for (int i = 0; i < NB64; ++i) {
    const int mb = wr + 2 * i;
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) ta[i][rd] = lds_base + (mb >> 2) * RP_PANEL + tr_off((mb & 3) * 32, rd);
  }
#pragma unroll
  for (int rd = 0; rd < 2; ++rd) tb[rd] = lds_base + NPAN * RP_PANEL + tr_off(wc * 32, rd);
  // ---- PE^T fragments of this wave's 32 columns, all k-chunks (lane: column n, buckets 16 c + 8 (lane >> 5) .. + 7), through the same
  // image: PE [nb][64] is copied to [nb rows][256 B] behind tile buffer 0 (buffer 1 and the staging slabs: both idle until the first
  // tile's barrier) and read transposed, 16 bucket rows = 4096 B per chunk.  (First form: 8 two-byte global loads per fragment, which
  // hipcc issued two at a time with a full wait in between -- 80 dependent round trips, ~30 us per block.)
  static_assert(NB * 256 <= BUF + RP_STAGE, "the PE image fits behind tile buffer 0");
  bf16x8 pef[NCH];
  {
#pragma unroll
    for (int i = 0; i < NB / 16; ++i) {
      const int row = (wave + 4 * i) * 4 + lrow;
      const bf16_t* src = lch < 8 ? pe + row * 64 + lch * 8 : zero;
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(dsm + BUF + wave * 1024 + i * 4096), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const unsigned p0 = lds_base + BUF + tr_off(wc * 32, 0), p1 = lds_base + BUF + tr_off(wc * 32, 1);
#pragma unroll
    for (int c = 0; c < NCH; ++c) pef[c] = rp_tr_frag(p0 + c * 4096, p1 + c * 4096);
    rp_lgkm_wait<0>();
#pragma unroll
    for (int c = 0; c < NCH; ++c) rp_tie(pef[c]);
  }   // (the first tile's barrier below is also the one between these reads and the next writes of that LDS)
  // row reads: row 32 wr + (lane & 31), chunk 2 (c & 7) + (lane >> 5) of panel c >> 3
  const int rrow = wr * 32 + (lane & 31);
  const int rmask = ((rrow & 3) << 2) | ((rrow >> 2) & 3);
  const unsigned ra = 256 * rrow + 16 * ((lane >> 5) ^ rmask);     // (chunk 2 (c & 7) + h: XOR 32 (c & 7) into the offset)

  f32x16 acc2[NB64];
#pragma unroll
  for (int i = 0; i < NB64; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[i][r] = 0.f;

  float* const stage = reinterpret_cast<float*>(dsm + 2 * BUF) + wave * (32 * RP_ST_LD);
  const int erow = lane >> 2, ecol = (lane & 3) * 8;       // epilogue: pass j covers row 16 j + erow, 8 columns from ecol

  // old dQ rows of this wave's tile, loaded one tile ahead: the loads go out in front of the next tile's DMA (loads return in order: behind
  // it they would wait for all of it) and are complete at the next tile's wait, so the epilogue waits for nothing and the DMA stays in
  // flight across it
  auto load_old = [&](const int tile, u32x4 (&o)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int t = tile * RP_TQ + wr * 32 + 16 * j + erow;
      t = t < T ? t : T - 1;       // (rows past T: a valid row, never used -- an unconditional load needs no wait where it is issued)
      o[j] = *reinterpret_cast<const u32x4*>(dq_z + (long long)t * dq_ld + wc * 32 + ecol);
    }
  };
  u32x4 old[2], old_next[2];
  load_old(0, old_next);

  for (int tile = 0; tile < ntiles; ++tile) {
    const int t0 = tile * RP_TQ;
    // vmcnt(0), the other counters left alone (the builtin, not inline assembly: the compiler's wait insertion has to see that old_next is in)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __builtin_amdgcn_s_barrier();
    old[0] = old_next[0]; old[1] = old_next[1];
    if (tile + 1 < ntiles) load_old(tile + 1, old_next);
    if (tile + 1 < ntiles) issue(tile + 1, (tile + 1) & 1);
    const unsigned cur = (tile & 1) * BUF;

    // ---- dPE partial: acc2[i] += dQP^T[32 buckets][16 t] . Q[16 t][32 columns], four k-chunks; the reads of chunk kg + 1 are issued in
    // front of the MFMAs of chunk kg
    if (want_part) {
      bf16x8 fa[2][NB64], fb[2];
#define RP_READ(S, KG)                                                                             \
  do {                                                                                             \
    fb[S] = rp_tr_frag(tb[0] + cur + (KG) * 4096, tb[1] + cur + (KG) * 4096);                      \
    _Pragma("unroll") for (int i = 0; i < NB64; ++i)                                               \
      fa[S][i] = rp_tr_frag(ta[i][0] + cur + (KG) * 4096, ta[i][1] + cur + (KG) * 4096);          \
  } while (0)
      RP_READ(0, 0);
#pragma unroll
      for (int kg = 0; kg < 4; ++kg) {
        const int s = kg & 1;
        if (kg < 3) { RP_READ(s ^ 1, kg + 1); rp_lgkm_wait<2 * (NB64 + 1)>(); }
        else rp_lgkm_wait<0>();
        rp_tie(fb[s]);
#pragma unroll
        for (int i = 0; i < NB64; ++i) rp_tie(fa[s][i]);
#pragma unroll
        for (int i = 0; i < NB64; ++i) acc2[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s][i], fb[s], acc2[i], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
#undef RP_READ
    }

    // ---- dQ tile: acc = dQP[32 t][nb] . PE[nb][32 columns], k-chunks in ascending order, four reads ahead
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    {
      bf16x8 fr[2][4];
#define RP_READ4(S, G)                                                                             \
  _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                  \
    const int c = (G) * 4 + e;                                                                     \
    fr[S][e] = rp_row_frag(lds_base + cur + (c >> 3) * RP_PANEL + (ra ^ (32 * (c & 7))));          \
  }
      RP_READ4(0, 0)
#pragma unroll
      for (int g = 0; g < NB64; ++g) {
        const int s = g & 1;
        if (g + 1 < NB64) { RP_READ4(s ^ 1, g + 1) rp_lgkm_wait<4>(); }
        else rp_lgkm_wait<0>();
#pragma unroll
        for (int e = 0; e < 4; ++e) rp_tie(fr[s][e]);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[s][e], pef[g * 4 + e], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
#undef RP_READ4
    }

    // ---- dQ epilogue through the wave's staging slab: 8 consecutive columns per lane, 16-byte stores
    {
      const int frow = lane & 31, fhalf = lane >> 5;
#pragma unroll
      for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * fhalf) * RP_ST_LD + frow] = acc[r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = 16 * j + erow;
        const int t = t0 + wr * 32 + row;
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(stage + row * RP_ST_LD + ecol);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(stage + row * RP_ST_LD + ecol + 4);
        if (t < T) {
          float x[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) { x[e] = x0[e] * alpha; x[4 + e] = x1[e] * alpha; }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            x[2 * e] = x[2 * e] + __uint_as_float(old[j][e] << 16);
            x[2 * e + 1] = x[2 * e + 1] + __uint_as_float(old[j][e] & 0xffff0000u);
          }
          store8f<bf16_t>(dq_z + (long long)t * dq_ld + wc * 32 + ecol, x);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the slab is rewritten by the next tile
    }
  }

  // ---- the partial: part[bh][bucket][column] = alpha * acc2, fp32 (lanes 0..31 of a register write 128 consecutive bytes)
  if (want_part) {
    float* const pz = part + (long long)bh * NB * 64 + wc * 32 + (lane & 31);
#pragma unroll
    for (int i = 0; i < NB64; ++i) {
      const int b0 = (wr + 2 * i) * 32 + 4 * (lane >> 5);
#pragma unroll
      for (int r = 0; r < 16; ++r) pz[(long long)(b0 + (r & 3) + 8 * (r >> 2)) * 64] = acc2[i][r] * alpha;
    }
  }
}

// dPE[c] = cast(sum over rows of part[r][c]) with the summation tree of colreduce_kernel<float, 0> + colreduce_final_kernel (norm.hip):
// nsplit = clamp(ceil(rows / 64), 1, 64) splits; inside split y eight running sums (ty takes rows y * 8 + ty, step nsplit * 8), added in the
// order ty = 0..7 from 0.f; the splits added in order from 0.f; times 1.0f; the conversion.  512 threads = 64 columns x 8 row lanes.
template <typename T>
__global__ __launch_bounds__(512) void relpos_dpe_final_kernel(const float* __restrict__ part, T* __restrict__ dpe, const long long rows,
                                                               const int cols, const int nsplit, const float* __restrict__ gate) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  if (st5_gate_dropped(gate)) {      // a dropped layer's gradient is read outside the layer: exact zeros, the partials are not read
    if (ty == 0 && c < cols) dpe[c] = Elem<T>::from_f(0.f);
    return;
  }
  __shared__ float red[2][8][64];
  float s = 0.f;
  for (int y = 0; y < nsplit; ++y) {
    float a = 0.f;
    if (c < cols)
      for (long long r = (long long)y * 8 + ty; r < rows; r += (long long)nsplit * 8) a += part[r * cols + c];
    red[y & 1][ty][tx] = a;
    __syncthreads();
    if (ty == 0) {
      float sy = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) sy += red[y & 1][j][tx];
      s += sy;
    }
  }
  if (ty == 0 && c < cols) {
    s *= 1.0f;
    dpe[c] = Elem<T>::from_f(s);
  }
}

template <int NB64>
int launch_relpos_bwd(const void* dqp, const void* q, long long q_ld, const void* pe, void* dq, long long dq_ld, float* part, int B, int H,
                      int T, float alpha, const float* gate, hipStream_t s) {
  constexpr size_t lds = 2 * ((NB64 + 1) / 2 + 1) * RP_PANEL + RP_STAGE;
  static_assert(lds <= 160 * 1024, "two tile buffers and the staging slabs fit the LDS");
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute((const void*)relpos_bwd_kernel<NB64>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return ST5_ERR_LAUNCH;
    attr = true;
  }
  hipLaunchKernelGGL(relpos_bwd_kernel<NB64>, dim3(B * H), dim3(256), lds, s, (const bf16_t*)dqp, (const bf16_t*)q, q_ld, (const bf16_t*)pe,
                     (bf16_t*)dq, dq_ld, part, H, T, alpha, gate);
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}

}  // namespace

extern "C" int st5_relpos_bwd_supported(int32_t nb) { return nb > 0 && nb % 64 == 0 && nb <= 320; }

extern "C" int st5_relpos_bwd(const void* dqp, const void* q, int64_t q_ld, const void* pe, void* dq, int64_t dq_ld, float* part, int32_t B,
                              int32_t H, int32_t T, int32_t nb, float alpha, const float* gate, int dtype, void* stream) {
  if (!dqp || !q || !pe || !dq || B <= 0 || H <= 0 || T <= 0 || dtype != ST5_BF16) return ST5_ERR_ARG;
  if (!st5_relpos_bwd_supported(nb) || q_ld < (int64_t)H * 64 || dq_ld < (int64_t)H * 64) return ST5_ERR_ARG;
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (!al16(dqp) || !al16(q) || !al16(dq) || !al16(part) || q_ld % 8 || dq_ld % 8) return ST5_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  switch (nb / 64) {
    case 1: return launch_relpos_bwd<1>(dqp, q, q_ld, pe, dq, dq_ld, part, B, H, T, alpha, gate, s);
    case 2: return launch_relpos_bwd<2>(dqp, q, q_ld, pe, dq, dq_ld, part, B, H, T, alpha, gate, s);
    case 3: return launch_relpos_bwd<3>(dqp, q, q_ld, pe, dq, dq_ld, part, B, H, T, alpha, gate, s);
    case 4: return launch_relpos_bwd<4>(dqp, q, q_ld, pe, dq, dq_ld, part, B, H, T, alpha, gate, s);
    default: return launch_relpos_bwd<5>(dqp, q, q_ld, pe, dq, dq_ld, part, B, H, T, alpha, gate, s);
  }
}

extern "C" int st5_relpos_dpe_final(const float* part, void* dpe, int64_t rows, int32_t cols, const float* gate, int dtype, void* stream) {
  if (!part || !dpe || rows <= 0 || cols <= 0) return ST5_ERR_ARG;
  long long ns = (rows + 63) / 64;
  ns = ns < 1 ? 1 : (ns > 64 ? 64 : ns);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((cols + 63) / 64);
  if (dtype == ST5_BF16)
    hipLaunchKernelGGL(relpos_dpe_final_kernel<bf16_t>, grid, dim3(512), 0, s, part, (bf16_t*)dpe, (long long)rows, cols, (int)ns, gate);
  else if (dtype == ST5_F32)
    hipLaunchKernelGGL(relpos_dpe_final_kernel<float>, grid, dim3(512), 0, s, part, (float*)dpe, (long long)rows, cols, (int)ns, gate);
  else return ST5_ERR_ARG;
  HIP_CHECK_LAUNCH();
  return ST5_OK;
}
