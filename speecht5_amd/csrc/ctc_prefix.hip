// CTC prefix scores for joint CTC / attention beam search (Watanabe et al. 2017, algorithm 2, many next labels at once).
// Follows what SpeechT5/speecht5/sequence_generator.py:273-418 calls once per hypothesis and step on the host
// (espnet CTCPrefixScore, in-tree copy Speech2C/speech2c/models/modules/ctc_prefix_score.py:10-112, numpy fp32):
//   r[t,0|1](h.c) = log r_t^n / r_t^b of prefix h extended by candidate c,   log_psi(h.c) = log prefix probability.
// Here every (hypothesis, candidate) pair of a step is one thread walking the T encoder frames; the CTC posterior x[T,V]
// and the per-hypothesis states stay on the device (the reference copies tokens and candidates to the host and loops in
// numpy per hypothesis).  The walk is a dependent chain of 3 log-add-exp per frame: latency-bound, ~T * 0.3 us per launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "ctc_rows_walk.h"
#include "../../include/speecht5_hip.h"

namespace {

using ctc_rows::LOGZERO;

// numpy's logaddexp for float32 (npy_logaddexpf): x + log1p(exp(-|x - y|)) on the larger operand
__device__ __forceinline__ float logaddexp(float a, float b) {
  if (a == b) return a + 0.693147180559945309417232121458176568f;
  const float d = a - b;
  return d > 0.f ? a + log1pf(expf(-d)) : b + log1pf(expf(d));
}

// cumulative blank path: r[t,1] = sum_{u<=t} x[u,blank], r[t,0] = logzero   (ctc_prefix_score.py:27-39)
__global__ void ctc_initial_state_kernel(const float* __restrict__ x, int T, int V, int blank, float* __restrict__ r) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float acc = 0.f;
  for (int t = 0; t < T; ++t) {
    acc = t == 0 ? x[blank] : acc + x[(long long)t * V + blank];
    r[2 * t] = LOGZERO;
    r[2 * t + 1] = acc;
  }
}

__global__ void ctc_prefix_score_kernel(const float* __restrict__ x, int T, int V, int blank, int eos,
                                        const float* __restrict__ r_prev, const long long* __restrict__ last,
                                        int out_len, const long long* __restrict__ cs, int nc,
                                        float* __restrict__ log_psi_out, float* __restrict__ r_new) {
  const int h = blockIdx.x, c = threadIdx.x;
  if (c >= nc) return;
  const long long tok = cs[(long long)h * nc + c];
  const float* rp = r_prev + (long long)h * T * 2;
  float* r = r_new + ((long long)h * nc + c) * T * 2;
  // the label that repeats the prefix's last one may only follow a blank: log_phi = r_prev^b instead of r^n + r^b (:66-72)
  const bool repeat = out_len > 0 && tok == last[h];
  const int start = out_len > 1 ? out_len : 1;
  for (int t = 0; t < start - 1; ++t) { r[2 * t] = LOGZERO; r[2 * t + 1] = LOGZERO; }   // (never read; numpy leaves them unset)
  float rn, rb;
  if (out_len == 0) { rn = x[tok]; rb = LOGZERO; }   // (:55-57)
  else { rn = LOGZERO; rb = LOGZERO; }               // (:59)
  if (start - 1 < T) { r[2 * (start - 1)] = rn; r[2 * (start - 1) + 1] = rb; }
  float log_psi = rn;                                 // (:78)
  for (int t = start; t < T; ++t) {
    const float pn = rp[2 * (t - 1)], pb = rp[2 * (t - 1) + 1];
    const float phi = repeat ? pb : logaddexp(pn, pb);
    const float xt = x[(long long)t * V + tok];
    const float nn = logaddexp(rn, phi) + xt;                               // (:80)
    const float nb = logaddexp(rn, rb) + x[(long long)t * V + blank];       // (:81-83)
    log_psi = logaddexp(log_psi, phi + xt);                                 // (:84)
    rn = nn; rb = nb;
    r[2 * t] = rn; r[2 * t + 1] = rb;
  }
  if (tok == eos) log_psi = logaddexp(rp[2 * (T - 1)], rp[2 * (T - 1) + 1]);   // P(... eos | X): the prefix itself ends (:87-89)
  if (tok == blank) log_psi = LOGZERO;                                           // (:92-94)
  log_psi_out[(long long)h * nc + c] = log_psi;
}


// ---------------------------------------------------------------------------------------------------------------------------------
// Rows form: a batch of sentences, each hypothesis row h scored against the posterior of ITS sentence sent[h] and that sentence's own
// frame count T_s = lens[sent[h]]  (x [S][Tmax][V] right-padded in time; no frame at or behind T_s is ever read).  The arithmetic
// of a (row, candidate) pair is that of ctc_prefix_score_kernel on x[s][:T_s]: same logaddexp, same order, same bits.  What differs:
//   * phi[t] depends on the row and the frame only: computed once per block, in parallel over t, into LDS (plain and repeat form;
//     only the candidate equal to last[h] takes the repeat form), together with the blank column.  Rows longer than ROWS_SEG frames
//     are walked in segments;
//   * the posterior gathers x[t][tok] are prefetched one chunk of ROWS_U frames ahead into registers, so the chain per frame is one
//     logaddexp on rn; the rb and log_psi updates hang off it;
//   * states are stored [nh][Tmax][nc][2]: the nc lanes of a block write consecutive bytes at each frame.  Frames at or behind T_s of
//     that buffer are not written (ctc_select_rows_kernel fills LOGZERO there when it gathers the continued hypotheses).
// out_len > T_s (a short sentence in a batch that decodes on): eos gets logaddexp(r_prev[T_s-1]) as always, every other candidate
// LOGZERO, the state is all LOGZERO.
// The walk of one pair is ctc_rows::walk (ctc_rows_walk.h), shared with the device-stepped form in beam_ctc.hip.

// r[s][t] = (LOGZERO, sum_{u<=t} x[s][u][blank]) for t < lens[s], summed in frame order; (LOGZERO, LOGZERO) behind
__global__ void ctc_initial_state_rows_kernel(const float* __restrict__ x, const int* __restrict__ lens, int Tmax, int V, int blank,
                                              float* __restrict__ r) {
  const int s = blockIdx.x;
  ctc_rows::initial_state(x + (long long)s * Tmax * V, lens[s], Tmax, V, blank, reinterpret_cast<float2*>(r) + (long long)s * Tmax);
}

__global__ void __launch_bounds__(1024)
ctc_prefix_score_rows_kernel(const float* __restrict__ x, const int* __restrict__ lens, const int* __restrict__ sent, int S, int Tmax,
                             int V, int blank, int eos, const float* __restrict__ r_prev, const long long* __restrict__ last,
                             int out_len, const long long* __restrict__ cs, int nc, float* __restrict__ log_psi_out,
                             float* __restrict__ r_new) {
  const int h = blockIdx.x, c = threadIdx.x;
  const bool live = c < nc;
  const int s = sent[h];
  int T = (s >= 0 && s < S) ? lens[s] : 0;
  T = T > Tmax ? Tmax : T;
  if (T <= 0) {                                         // (a row without a sentence or without frames: nothing to read)
    if (live) log_psi_out[(long long)h * nc + c] = LOGZERO;
    return;
  }
  const long long tok = live ? cs[(long long)h * nc + c] : (long long)blank;
  const float log_psi = ctc_rows::walk(x + (long long)s * Tmax * V, T, V, blank, eos, r_prev + (long long)h * Tmax * 2,
                                       out_len > 0 && tok == last[h], out_len, tok, live, nc,
                                       reinterpret_cast<float2*>(r_new) + (long long)h * Tmax * nc + c);
  if (live) log_psi_out[(long long)h * nc + c] = log_psi;
}

// Next step's prefix state of each continued hypothesis n: the extension (parent[n], slot of token[n] in cs[parent[n]]) of this
// step's launch, gathered from the [nh][Tmax][nc][2] buffer; LOGZERO at and behind the sentence's frame count.  A token outside the
// candidate list: known = 0, slot 0 is gathered (the caller raises).  sent_out (may be NULL): the sentence of the parent row.
constexpr int SELECT_THREADS = 256;

__global__ void __launch_bounds__(SELECT_THREADS)
ctc_select_rows_kernel(const int* __restrict__ lens, const int* __restrict__ sent, int S, int Tmax, const long long* __restrict__ cs,
                       int nh, int nc, const float* __restrict__ log_psi, const float* __restrict__ r_new,
                       const long long* __restrict__ parent, const long long* __restrict__ token, float* __restrict__ state,
                       float* __restrict__ prev_psi, unsigned char* __restrict__ known, int* __restrict__ sent_out) {
  __shared__ int slot_s[SELECT_THREADS];
  const int n = blockIdx.x;
  const long long p = parent[n];
  float2* st = reinterpret_cast<float2*>(state) + (long long)n * Tmax;
  const int s = (p >= 0 && p < nh) ? sent[p] : -1;
  int T = (s >= 0 && s < S) ? lens[s] : 0;
  T = T < 0 ? 0 : (T > Tmax ? Tmax : T);
  if (T == 0) {                                         // (a parent outside the launch: nothing to gather)
    for (int t = threadIdx.x; t < Tmax; t += SELECT_THREADS) st[t] = make_float2(LOGZERO, LOGZERO);
    if (threadIdx.x == 0) { prev_psi[n] = LOGZERO; known[n] = 0; if (sent_out) sent_out[n] = s; }
    return;
  }
  const long long tok = token[n];
  int slot = nc;
  for (int c = threadIdx.x; c < nc; c += SELECT_THREADS)
    if (cs[p * nc + c] == tok && c < slot) slot = c;
  slot_s[threadIdx.x] = slot;
  __syncthreads();
  for (int w = SELECT_THREADS / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) { const int o = slot_s[threadIdx.x + w]; if (o < slot_s[threadIdx.x]) slot_s[threadIdx.x] = o; }
    __syncthreads();
  }
  slot = slot_s[0];
  const bool found = slot < nc;
  if (!found) slot = 0;
  const float2* src = reinterpret_cast<const float2*>(r_new) + p * Tmax * nc + slot;
  for (int t = threadIdx.x; t < Tmax; t += SELECT_THREADS) st[t] = t < T ? src[(long long)t * nc] : make_float2(LOGZERO, LOGZERO);
  if (threadIdx.x == 0) {
    prev_psi[n] = log_psi[p * nc + slot];
    known[n] = found ? 1 : 0;
    if (sent_out) sent_out[n] = s;
  }
}

}  // namespace

extern "C" int st5_ctc_initial_state(const float* x, int T, int V, int blank, float* r, void* stream) {
  if (!x || !r || T <= 0 || V <= 0 || blank < 0 || blank >= V) return ST5_ERR_ARG;
  hipLaunchKernelGGL(ctc_initial_state_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), x, T, V, blank, r);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_ctc_prefix_score(const float* x, int T, int V, int blank, int eos, const float* r_prev, const int64_t* last,
                                    int out_len, const int64_t* cs, int nh, int nc, float* log_psi, float* r_new, void* stream) {
  if (!x || !r_prev || !last || !cs || !log_psi || !r_new) return ST5_ERR_ARG;
  if (T <= 0 || V <= 0 || nh <= 0 || nc <= 0 || nc > 1024 || out_len < 0 || out_len > T) return ST5_ERR_ARG;
  if (blank < 0 || blank >= V || eos < 0 || eos >= V) return ST5_ERR_ARG;
  const int threads = (nc + 63) / 64 * 64;
  hipLaunchKernelGGL(ctc_prefix_score_kernel, dim3(nh), dim3(threads), 0, reinterpret_cast<hipStream_t>(stream), x, T, V, blank, eos,
                     r_prev, reinterpret_cast<const long long*>(last), out_len, reinterpret_cast<const long long*>(cs), nc, log_psi,
                     r_new);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_ctc_initial_state_rows(const float* x, const int32_t* lens, int S, int Tmax, int V, int blank, float* r, void* stream) {
  if (!x || !lens || !r || S <= 0 || Tmax <= 0 || V <= 0 || blank < 0 || blank >= V) return ST5_ERR_ARG;
  hipLaunchKernelGGL(ctc_initial_state_rows_kernel, dim3(S), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), x, lens, Tmax, V, blank, r);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_ctc_prefix_score_rows(const float* x, const int32_t* lens, const int32_t* sent, int S, int Tmax, int V, int blank,
                                         int eos, const float* r_prev, const int64_t* last, int out_len, const int64_t* cs, int nh,
                                         int nc, float* log_psi, float* r_new, void* stream) {
  if (!x || !lens || !sent || !r_prev || !last || !cs || !log_psi || !r_new) return ST5_ERR_ARG;
  if (S <= 0 || Tmax <= 0 || V <= 0 || nh <= 0 || nc <= 0 || nc > 1024 || out_len < 0) return ST5_ERR_ARG;
  if (blank < 0 || blank >= V || eos < 0 || eos >= V) return ST5_ERR_ARG;
  const int threads = (nc + 63) / 64 * 64;
  hipLaunchKernelGGL(ctc_prefix_score_rows_kernel, dim3(nh), dim3(threads), 0, reinterpret_cast<hipStream_t>(stream), x, lens, sent, S,
                     Tmax, V, blank, eos, r_prev, reinterpret_cast<const long long*>(last), out_len,
                     reinterpret_cast<const long long*>(cs), nc, log_psi, r_new);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_ctc_select_rows(const int32_t* lens, const int32_t* sent, int S, int Tmax, const int64_t* cs, int nh, int nc,
                                   const float* log_psi, const float* r_new, const int64_t* parent, const int64_t* token, int n,
                                   float* state, float* prev_psi, uint8_t* known, int32_t* sent_out, void* stream) {
  if (!lens || !sent || !cs || !log_psi || !r_new || !parent || !token || !state || !prev_psi || !known) return ST5_ERR_ARG;
  if (S <= 0 || Tmax <= 0 || nh <= 0 || nc <= 0 || nc > 1024 || n <= 0) return ST5_ERR_ARG;
  hipLaunchKernelGGL(ctc_select_rows_kernel, dim3(n), dim3(SELECT_THREADS), 0, reinterpret_cast<hipStream_t>(stream), lens, sent, S, Tmax,
                     reinterpret_cast<const long long*>(cs), nh, nc, log_psi, r_new, reinterpret_cast<const long long*>(parent),
                     reinterpret_cast<const long long*>(token), state, prev_psi, known, sent_out);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}
