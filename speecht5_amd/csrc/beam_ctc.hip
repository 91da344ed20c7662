// Joint CTC / attention scoring inside a device-stepped beam search step (SequenceGenerator(decode="device" / "graph", ctc_weight > 0,
// ctc_rows=True), speecht5_amd/beam_graph.py): what the generator does between the decoder's output and the beam search step
// (sequence_generator.py _generate: topk of the candidates, CTCPrefixScorerRows.score, the mix, .select), for the step held in the
// int32 device counter of beam_step.hip.  Row r belongs to sentence r / beam for the whole call.  Per step, in launch order:
//   st5_beam_ctc_candidates (in front of the scorer), step = *counter:
//     lp[r][c] = (logits[r][c] / temperature - mx) - lse, the statistics and the expression of beam_step_kernel stage 1, unruled;
//     cs[r][0 .. nc) = the nc best tokens of lp[r] with never[c] tokens and NaN taken as -inf, in rank order: higher value first, among
//     equal values the lower token first (radix select on the unique key of beam_select.h).
//   st5_ctc_prefix_score_rows_dev: ctc_prefix_score_rows_kernel's walk (ctc_rows_walk.h) with out_len = step, last = tok[r][step] and
//     int32 candidates, then the mix lp[r][cs[r][j]] = (float)(1 - w) * lp + (float)w * (log_psi[r][j] - prev[r]), each operation
//     rounded to fp32 on its own (the generator's torch expression).
//   st5_beam_step_logprobs (beam_step.hip) on lp; it advances the counter.
//   st5_ctc_select_dev, t = *counter, 1 <= t <= max_len: row r continues parent[r] with tok[r][t]; state[r] and prev[r] are gathered
//     from the parent's extension by that token.  A token outside cs[parent]: slot 0 is gathered and *unknown = 1, unless the row is
//     ignored or its sentence finished (those rows keep running and mean nothing).
// Every index read from device memory is range-checked before it is used; a bad one shows up as NaN / LOGZERO state and a set
// `unknown`, it is never dereferenced.  Plain vector loads and stores only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "beam_select.h"
#include "ctc_rows_walk.h"
#include "../../include/speecht5_hip.h"

namespace {

using bsel::u64;
using ctc_rows::LOGZERO;

constexpr int CAND_MAX = 1024;            // candidates per row: the scorer's one-block-per-row limit

__global__ void __launch_bounds__(bsel::THREADS)
beam_ctc_candidates_kernel(const float* __restrict__ logits, int64_t ld, int V, float temperature, const uint8_t* __restrict__ never,
                           const int32_t* __restrict__ counter, int max_len, float* __restrict__ lp, int64_t lp_ld,
                           int32_t* __restrict__ cs, int nc) {
  const int step = *counter;
  if (step < 0 || step > max_len) return;
  const int r = blockIdx.x, tid = threadIdx.x;
  __shared__ float s_mx, s_lse;
  __shared__ u64 s_sorted[CAND_MAX];
  const float* x = logits + (int64_t)r * ld;
  float* out = lp + (int64_t)r * lp_ld;
  if (tid < 64) {                          // one wave, as in beam_step_kernel: the same order of the reductions, the same bits
    float mx, lse;
    bsel::row_stats(x, V, temperature, tid, mx, lse);
    if (tid == 0) { s_mx = mx; s_lse = lse; }
  }
  bsel::sync();
  const float mx = s_mx, lse = s_lse;
  // thread tid owns the columns tid + k * THREADS here and in the selection: it reads back what it wrote itself
  for (int c = tid; c < V; c += bsel::THREADS) out[c] = (x[c] / temperature - mx) - lse;
  const int nsel = bsel::select_top<CAND_MAX>(
      [&](int, int c) {
        float v = out[c];
        if (v != v || never[c]) v = -INFINITY;
        return ((u64)bsel::fkey(v) << 32) | (uint32_t)(~(uint32_t)c);
      },
      1, V, nc, s_sorted);
  for (int j = tid; j < nc; j += bsel::THREADS) cs[(int64_t)r * nc + j] = j < nsel ? (int32_t)(~(uint32_t)s_sorted[j]) : -1;
}

// the generator's (1 - w) * lprobs + w * (log_psi - prev) in fp32: two products and a sum, each rounded on its own (no fused
// multiply-add: torch's expression has none)
__device__ __forceinline__ float ctc_mix(float w_att, float lp, float w_ctc, float log_psi, float prev) {
#pragma clang fp contract(off)
  const float a = w_att * lp;
  const float b = w_ctc * (log_psi - prev);
  return a + b;
}

__global__ void __launch_bounds__(1024)
ctc_prefix_score_rows_dev_kernel(const float* __restrict__ x, const int* __restrict__ lens, int S, int Tfr, int V, int blank, int eos,
                                 int beam, const float* __restrict__ r_prev, const int32_t* __restrict__ tok, int tok_ld,
                                 const int32_t* __restrict__ counter, int max_len, const int32_t* __restrict__ cs, int nc,
                                 float* __restrict__ log_psi_out, float* __restrict__ r_new, const float* __restrict__ prev,
                                 float* __restrict__ lp, int64_t lp_ld, float w_att, float w_ctc) {
  const int step = *counter;
  if (step < 0 || step > max_len) return;
  const int h = blockIdx.x, c = threadIdx.x;
  const bool live = c < nc;
  const int s = h / beam;
  int T = s < S ? lens[s] : 0;
  T = T > Tfr ? Tfr : T;
  const int32_t cand = live ? cs[(int64_t)h * nc + c] : blank;
  const bool ok = cand >= 0 && cand < V;
  const long long t = ok ? cand : blank;
  float log_psi = LOGZERO;
  if (T > 0)                               // (block-uniform.  A sentence without frames: nothing to read, every extension is impossible)
    log_psi = ctc_rows::walk(x + (long long)s * Tfr * V, T, V, blank, eos, r_prev + (long long)h * Tfr * 2,
                             step > 0 && t == (long long)tok[(int64_t)h * tok_ld + step], step, t, live, nc,
                             reinterpret_cast<float2*>(r_new) + (long long)h * Tfr * nc + c);
  if (!live) return;
  log_psi_out[(int64_t)h * nc + c] = ok ? log_psi : NAN;
  if (ok) {
    float* p = lp + (int64_t)h * lp_ld + t;
    *p = ctc_mix(w_att, *p, w_ctc, log_psi, prev[h]);
  }
}

constexpr int SELECT_THREADS = 256;

__global__ void __launch_bounds__(SELECT_THREADS)
ctc_select_dev_kernel(const int* __restrict__ lens, int S, int Tfr, int beam, int rows, const int32_t* __restrict__ cs, int nc,
                      const float* __restrict__ log_psi, const float* __restrict__ r_new, const int32_t* __restrict__ parent,
                      const int32_t* __restrict__ tok, int tok_ld, const uint8_t* __restrict__ ignore,
                      const int32_t* __restrict__ sent_done, const int32_t* __restrict__ counter, int max_len,
                      float* __restrict__ state, float* __restrict__ prev, int32_t* __restrict__ unknown) {
  const int t = *counter;
  if (t < 1 || t > max_len) return;
  __shared__ int slot_s[SELECT_THREADS];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int s = n / beam;
  const int p = parent[n];
  float2* st = reinterpret_cast<float2*>(state) + (int64_t)n * Tfr;
  const bool counts = !ignore[n] && !(s < S && sent_done[s]);
  if (p < 0 || p >= rows) {                // (a broken parent: no state, and the host hears of it)
    for (int f = tid; f < Tfr; f += SELECT_THREADS) st[f] = make_float2(LOGZERO, LOGZERO);
    if (tid == 0) { prev[n] = NAN; if (counts) *unknown = 1; }
    return;
  }
  int T = s < S ? lens[s] : 0;
  T = T < 0 ? 0 : (T > Tfr ? Tfr : T);
  const int32_t token = tok[(int64_t)n * tok_ld + t];
  int slot = nc;
  for (int c = tid; c < nc; c += SELECT_THREADS)
    if (cs[(int64_t)p * nc + c] == token && c < slot) slot = c;
  slot_s[tid] = slot;
  bsel::sync();
  for (int w = SELECT_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) { const int o = slot_s[tid + w]; if (o < slot_s[tid]) slot_s[tid] = o; }
    bsel::sync();
  }
  slot = slot_s[0];
  const bool found = slot < nc;
  if (!found) slot = 0;
  const float2* src = reinterpret_cast<const float2*>(r_new) + (int64_t)p * Tfr * nc + slot;
  for (int f = tid; f < Tfr; f += SELECT_THREADS) st[f] = f < T ? src[(int64_t)f * nc] : make_float2(LOGZERO, LOGZERO);
  if (tid == 0) {
    prev[n] = log_psi[(int64_t)p * nc + slot];
    if (!found && counts) *unknown = 1;
  }
}

}  // namespace

extern "C" int st5_beam_ctc_candidates(const float* logits, int64_t ld, int32_t rows, int32_t V, float temperature, const uint8_t* never,
                                       const int32_t* counter, int32_t max_len, float* lp, int64_t lp_ld, int32_t* cs, int32_t nc,
                                       void* stream) {
  if (!logits || !never || !counter || !lp || !cs) return ST5_ERR_ARG;
  if (rows <= 0 || V <= 0 || nc <= 0 || nc > CAND_MAX || nc > V || ld < V || lp_ld < V || max_len < 0 || !(temperature > 0.f))
    return ST5_ERR_ARG;
  hipLaunchKernelGGL(beam_ctc_candidates_kernel, dim3(rows), dim3(bsel::THREADS), 0, reinterpret_cast<hipStream_t>(stream), logits, ld, V,
                     temperature, never, counter, max_len, lp, lp_ld, cs, nc);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_ctc_prefix_score_rows_dev(const float* x, const int32_t* lens, int32_t S, int32_t Tfr, int32_t V, int32_t blank,
                                             int32_t eos, int32_t beam, const float* r_prev, const int32_t* tok, int32_t tok_ld,
                                             const int32_t* counter, int32_t max_len, const int32_t* cs, int32_t nc, float* log_psi,
                                             float* r_new, const float* prev, float* lp, int64_t lp_ld, double ctc_weight, void* stream) {
  if (!x || !lens || !r_prev || !tok || !counter || !cs || !log_psi || !r_new || !prev || !lp) return ST5_ERR_ARG;
  if (S <= 0 || Tfr <= 0 || V <= 0 || beam <= 0 || nc <= 0 || nc > CAND_MAX || (int64_t)S * beam > 0x7fffffffll) return ST5_ERR_ARG;
  if (blank < 0 || blank >= V || eos < 0 || eos >= V || max_len < 0 || tok_ld < max_len + 1 || lp_ld < V) return ST5_ERR_ARG;
  if (!(ctc_weight >= 0.0 && ctc_weight <= 1.0)) return ST5_ERR_ARG;
  const int threads = (nc + 63) / 64 * 64;
  hipLaunchKernelGGL(ctc_prefix_score_rows_dev_kernel, dim3(S * beam), dim3(threads), 0, reinterpret_cast<hipStream_t>(stream), x, lens, S,
                     Tfr, V, blank, eos, beam, r_prev, tok, tok_ld, counter, max_len, cs, nc, log_psi, r_new, prev, lp, lp_ld,
                     (float)(1.0 - ctc_weight), (float)ctc_weight);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_ctc_select_dev(const int32_t* lens, int32_t S, int32_t Tfr, int32_t beam, const int32_t* cs, int32_t nc,
                                  const float* log_psi, const float* r_new, const int32_t* parent, const int32_t* tok, int32_t tok_ld,
                                  const uint8_t* ignore, const int32_t* sent_done, const int32_t* counter, int32_t max_len, float* state,
                                  float* prev, int32_t* unknown, void* stream) {
  if (!lens || !cs || !log_psi || !r_new || !parent || !tok || !ignore || !sent_done || !counter || !state || !prev || !unknown)
    return ST5_ERR_ARG;
  if (S <= 0 || Tfr <= 0 || beam <= 0 || nc <= 0 || nc > CAND_MAX || (int64_t)S * beam > 0x7fffffffll) return ST5_ERR_ARG;
  if (max_len < 0 || tok_ld < max_len + 1) return ST5_ERR_ARG;
  hipLaunchKernelGGL(ctc_select_dev_kernel, dim3(S * beam), dim3(SELECT_THREADS), 0, reinterpret_cast<hipStream_t>(stream), lens, S, Tfr,
                     beam, S * beam, cs, nc, log_psi, r_new, parent, tok, tok_ld, ignore, sent_done, counter, max_len, state, prev, unknown);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}
