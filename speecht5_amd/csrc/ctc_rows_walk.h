// The frame walk of the rows form of the CTC prefix scorer, shared by ctc_prefix_score_rows_kernel (ctc_prefix.hip: out_len and the
// indices from the host) and ctc_prefix_score_rows_dev_kernel (beam_ctc.hip: the step from a device counter): one copy of the
// arithmetic, so the two give the same bits.  See the "Rows form" note in ctc_prefix.hip for what the walk does and why.
#pragma once
#include <hip/hip_runtime.h>

namespace ctc_rows {

constexpr float LOGZERO = -10000000000.0f;   // ctc_prefix_score.py:21

// logaddexp without the branches: the larger operand and -|a - b| are selected, then ONE log1pf(expf()) serves both orders.  The
// same operations on the same values as numpy's logaddexp (ctc_prefix.hip) in every case (d > 0: a + log1pf(expf(-d)); else
// b + log1pf(expf(d)); a == b: a + ln 2), hence the same bits; straight-line code lets the three recursions of a frame overlap in the
// pipeline, where the branchy form runs them one after the other and, in a wave whose lanes disagree on the order, both sides of each.
__device__ __forceinline__ float logaddexp_sel(float a, float b) {
  const float d = a - b;
  const bool gt = d > 0.f;
  const float g = (gt ? a : b) + log1pf(expf(gt ? -d : d));
  return a == b ? a + 0.693147180559945309417232121458176568f : g;
}

// The initial prefix state of one sentence, by the threads of one block: rs[t] = (LOGZERO, sum_{u<=t} xs[u][blank]) for t < T, summed
// in frame order by thread 0; (LOGZERO, LOGZERO) for T <= t < Tmax.  T is brought into [0, Tmax] here.  Shared by
// ctc_initial_state_rows_kernel (ctc_prefix.hip) and the stream's admission (beam_ctc.hip: ctc_sents_admit_kernel).
__device__ __forceinline__ void initial_state(const float* __restrict__ xs, int T, int Tmax, int V, int blank, float2* __restrict__ rs) {
  T = T < 0 ? 0 : (T > Tmax ? Tmax : T);
  for (int t = T + threadIdx.x; t < Tmax; t += blockDim.x) rs[t] = make_float2(LOGZERO, LOGZERO);
  if (threadIdx.x != 0) return;
  float acc = 0.f;
  for (int t = 0; t < T; ++t) {
    acc = t == 0 ? xs[blank] : acc + xs[(long long)t * V + blank];
    rs[t] = make_float2(LOGZERO, acc);
  }
}

constexpr int ROWS_SEG = 2048;            // frames per LDS segment
constexpr int ROWS_U = 16;                // frames per prefetched chunk
constexpr int ROWS_REP = ROWS_SEG + 4;    // offset of the repeat form in phi_s (+4: the two forms never share a bank slot)

// One (row, candidate) pair: thread threadIdx.x of the row's block extends the prefix with state rp [T][2] by `tok` over the T > 0
// frames xs [T][V] of the row's sentence, writes the extension's state to r[t * nc] for t < T (live threads) and returns log_psi.
// EVERY thread of the block calls it with the same xs, T, rp, out_len (block barriers inside); threads past the candidate list pass
// live = false and tok = blank.
__device__ __forceinline__ float walk(const float* __restrict__ xs, int T, int V, int blank, int eos, const float* __restrict__ rp,
                                      bool repeat, int out_len, long long tok, bool live, int nc, float2* __restrict__ r) {
  __shared__ __attribute__((aligned(16))) float phi_s[ROWS_REP + ROWS_SEG];
  __shared__ __attribute__((aligned(16))) float xb_s[ROWS_SEG];
  const int po = repeat ? ROWS_REP : 0;
  const int start = out_len > 1 ? out_len : 1;
  const int head = start - 1 < T ? start - 1 : T;
  if (live)
    for (int t = 0; t < head; ++t) r[(long long)t * nc] = make_float2(LOGZERO, LOGZERO);
  float rn, rb;
  if (out_len == 0) { rn = xs[tok]; rb = LOGZERO; }
  else { rn = LOGZERO; rb = LOGZERO; }
  if (start - 1 < T && live) r[(long long)(start - 1) * nc] = make_float2(rn, rb);
  float log_psi = rn;
  for (int t0 = start; t0 < T; t0 += ROWS_SEG) {        // (block-uniform trip count)
    const int n = T - t0 < ROWS_SEG ? T - t0 : ROWS_SEG;
    __syncthreads();                                    // the previous segment has been walked
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
      const int t = t0 + j;
      const float pn = rp[2 * (t - 1)], pb = rp[2 * (t - 1) + 1];
      phi_s[j] = logaddexp_sel(pn, pb);
      phi_s[ROWS_REP + j] = pb;
      xb_s[j] = xs[(long long)t * V + blank];
    }
    __syncthreads();
    if (live) {
      const float* xt_p = xs + (long long)t0 * V + tok;
      float2* rt = r + (long long)t0 * nc;
      float xa[ROWS_U];
#pragma unroll
      for (int u = 0; u < ROWS_U; ++u) xa[u] = u < n ? xt_p[(long long)u * V] : 0.f;
      for (int j0 = 0; j0 < n; j0 += ROWS_U) {
        float xn[ROWS_U];
#pragma unroll
        for (int u = 0; u < ROWS_U; ++u) {              // the next chunk's gathers fly while this chunk is walked
          const int jn = j0 + ROWS_U + u;
          xn[u] = jn < n ? xt_p[(long long)jn * V] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < ROWS_U; ++u) {
          const int j = j0 + u;
          if (j < n) {
            const float phi = phi_s[po + j];
            const float xt = xa[u];
            const float nn = logaddexp_sel(rn, phi) + xt;
            const float nb = logaddexp_sel(rn, rb) + xb_s[j];
            log_psi = logaddexp_sel(log_psi, phi + xt);
            rn = nn; rb = nb;
            rt[(long long)j * nc] = make_float2(rn, rb);
          }
        }
#pragma unroll
        for (int u = 0; u < ROWS_U; ++u) xa[u] = xn[u];
      }
    }
  }
  if (tok == eos) log_psi = logaddexp_sel(rp[2 * (T - 1)], rp[2 * (T - 1) + 1]);
  if (tok == blank) log_psi = LOGZERO;
  return log_psi;
}

}  // namespace ctc_rows
