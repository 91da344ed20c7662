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
// The per-slot forms (the step of a beam-search stream with joint_ctc, speecht5_amd/beam_stream.py; index arithmetic:
// beam_stream_index.h) are the same kernel bodies under a template flag, as beam_step_kernel<SENTS> is: slot s = r / beam reads its own
// step pos[s], limit maxlen[s], done[s], moved[s] and frame count frames[s] where the scalar forms read one counter, one max_len and
// the call's lens.  The posterior is x [n_slots][S][V]; ctc_rows::walk and ctc_mix are used as they are, so the bits per (row,
// candidate) pair are the scalar forms'.
//   st5_beam_ctc_candidates_sents / st5_ctc_prefix_score_rows_sents: a slot that is done, or whose step is not live, returns before its
//     first load and writes nothing.
//   st5_ctc_select_sents: acts only where the beam step in front of it moved the slot, at t = pos[s]; `unknown` is int32 [n_slots], set
//     by a row that still counts (not ignored, its slot not done behind the step); a parent must lie inside the row's own slot.
//   st5_ctc_sents_admit: behind st5_beam_sents_admit, over the same descriptors: frames[slot], the slot's prefix states (the initial
//     state of its posterior over its own frames, ctc_rows::initial_state, LOGZERO behind them), prev = 0, unknown[slot] = 0.
// No kernel here writes done, pos or anything of another slot, and none reads another slot's CTC state.
// Every index read from device memory is range-checked before it is used; a bad one shows up as NaN / LOGZERO state and a set
// `unknown`, it is never dereferenced.  Plain vector loads and stores only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "beam_select.h"
#include "ctc_rows_walk.h"
#include "beam_stream_index.h"
#include "../../include/speecht5_hip.h"

namespace {

using bsel::u64;
using ctc_rows::LOGZERO;

constexpr int CAND_MAX = 1024;            // candidates per row: the scorer's one-block-per-row limit

// Where a kernel takes its step from, as beam_reorder_dev_kernel<SENTS> does it: `counter` and `max_len` are the launch's one counter
// and one limit (X = CtcScalar), or the stream's pos [n_slots] and its cap with the rest of the slot state in X = CtcSents: slot
// s = row / beam has its own pos[s], maxlen[s] (clamped into [0, cap]), done[s], moved[s] (BeamStreamState; null where not read).
struct CtcScalar {};
struct CtcSents { const int32_t* maxlen; const int32_t* done; const int32_t* moved; int beam; };

// the step a row's workgroup scores, in front of the beam step; false: the workgroup returns before its first load.  Uniform per
// workgroup (one workgroup per row, every thread reads the same cells).
template <bool SENTS, typename X>
__device__ __forceinline__ bool ctc_step_of(const int32_t* __restrict__ counter, int max_len, const X& x, int row, int& step) {
  if constexpr (SENTS) {
    const int s = (int)bst_slot_of(row, x.beam);
    step = counter[s];
    return bst_ctc_live(x.done[s], step, bst_maxlen(x.maxlen[s], max_len));
  } else {
    step = *counter;
    return step >= 0 && step <= max_len;
  }
}

template <bool SENTS, typename X>
__global__ void __launch_bounds__(bsel::THREADS)
beam_ctc_candidates_kernel(const float* __restrict__ logits, int64_t ld, int V, float temperature, const uint8_t* __restrict__ never,
                           const int32_t* __restrict__ counter, int max_len, float* __restrict__ lp, int64_t lp_ld,
                           int32_t* __restrict__ cs, int nc, const X sx) {
  int step;
  if (!ctc_step_of<SENTS>(counter, max_len, sx, blockIdx.x, step)) return;
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

// SENTS: lens is the stream's frames [n_slots], S its n_slots and Tfr its encoder positions per slot, so T = clamp(frames[s], 0, Tfr),
// out_len = pos[s], last = tok[r][pos[s]].  The gate is uniform per workgroup (one workgroup per row; pos, maxlen and done of the row's
// slot are the same cells for every thread), and so is T: the barriers inside ctc_rows::walk stay uniform.
template <bool SENTS, typename X>
__global__ void __launch_bounds__(1024)
ctc_prefix_score_rows_dev_kernel(const float* __restrict__ x, const int* __restrict__ lens, int S, int Tfr, int V, int blank, int eos,
                                 int beam, const float* __restrict__ r_prev, const int32_t* __restrict__ tok, int tok_ld,
                                 const int32_t* __restrict__ counter, int max_len, const int32_t* __restrict__ cs, int nc,
                                 float* __restrict__ log_psi_out, float* __restrict__ r_new, const float* __restrict__ prev,
                                 float* __restrict__ lp, int64_t lp_ld, float w_att, float w_ctc, const X sx) {
  int step_;
  if (!ctc_step_of<SENTS>(counter, max_len, sx, blockIdx.x, step_)) return;
  const int step = step_;
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

// SENTS: only the slots the beam step in front moved, at t = pos[s] under maxlen[s]; sent_done is the stream's `done` as that step
// left it, `unknown` is per slot, and a parent outside the row's own slot is a broken parent.  Row n writes state[n], prev[n] and its
// own slot's flag, nothing else.
template <bool SENTS, typename X>
__global__ void __launch_bounds__(SELECT_THREADS)
ctc_select_dev_kernel(const int* __restrict__ lens, int S, int Tfr, int beam, int rows, const int32_t* __restrict__ cs, int nc,
                      const float* __restrict__ log_psi, const float* __restrict__ r_new, const int32_t* __restrict__ parent,
                      const int32_t* __restrict__ tok, int tok_ld, const uint8_t* __restrict__ ignore,
                      const int32_t* __restrict__ sent_done, const int32_t* __restrict__ counter, int max_len,
                      float* __restrict__ state, float* __restrict__ prev, int32_t* __restrict__ unknown, const X sx) {
  int t_;
  if constexpr (SENTS) {
    const int sl = (int)bst_slot_of(blockIdx.x, beam);
    t_ = counter[sl];
    if (!bst_select_live(sx.moved[sl], t_, bst_maxlen(sx.maxlen[sl], max_len))) return;
  } else {
    t_ = *counter;
    if (t_ < 1 || t_ > max_len) return;
  }
  const int t = t_;
  __shared__ int slot_s[SELECT_THREADS];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int s = n / beam;
  const int p = parent[n];
  float2* st = reinterpret_cast<float2*>(state) + (int64_t)n * Tfr;
  const bool counts = !ignore[n] && !(s < S && sent_done[s]);
  int32_t* flag = SENTS ? unknown + s : unknown;
  if (SENTS ? !bst_parent_ok(p, s, beam) : (p < 0 || p >= rows)) {   // (a broken parent: no state, and the host hears of it)
    for (int f = tid; f < Tfr; f += SELECT_THREADS) st[f] = make_float2(LOGZERO, LOGZERO);
    if (tid == 0) { prev[n] = NAN; if (counts) *flag = 1; }
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
    if (!found && counts) *flag = 1;
  }
}

// grid (n_admit) over st5_beam_sents_admit's descriptors (slot, max_len, frames, bos): workgroup i gives slot desc[i][0] the CTC state of
// a new sentence whose posterior lies in the slot's slice of x.  A slot outside [0, n_slots) admits nothing; every write lies inside
// the slot's rows / its own cells of frames and unknown.
constexpr int ADMIT_THREADS = 256;

__global__ void __launch_bounds__(ADMIT_THREADS)
ctc_sents_admit_kernel(const int32_t* __restrict__ desc, int n_slots, int beam, const float* __restrict__ x, int S, int V, int blank,
                       int32_t* __restrict__ frames, float* __restrict__ state, float* __restrict__ prev, int32_t* __restrict__ unknown) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int slot = desc[4 * i];
  if (!bst_slot_ok(slot, n_slots)) return;
  const int T = bst_frames(desc[4 * i + 2], S);
  const int64_t row0 = bst_row0(slot, beam);
  float2* st0 = reinterpret_cast<float2*>(state) + bst_state_off(row0, S);
  ctc_rows::initial_state(x + bst_x_off(slot, S, V), T, S, V, blank, st0);
  __syncthreads();                         // (row0's state, written by this workgroup, is read back below)
  for (int e = tid; e < (beam - 1) * S; e += ADMIT_THREADS) {
    const int b = 1 + e / S, f = e % S;
    reinterpret_cast<float2*>(state)[bst_state_off(row0 + b, S) + f] = st0[f];
  }
  for (int b = tid; b < beam; b += ADMIT_THREADS) prev[row0 + b] = 0.f;
  if (tid == 0) {
    frames[slot] = T;
    unknown[slot] = 0;
  }
}

}  // namespace

extern "C" int st5_beam_ctc_candidates(const float* logits, int64_t ld, int32_t rows, int32_t V, float temperature, const uint8_t* never,
                                       const int32_t* counter, int32_t max_len, float* lp, int64_t lp_ld, int32_t* cs, int32_t nc,
                                       void* stream) {
  if (!logits || !never || !counter || !lp || !cs) return ST5_ERR_ARG;
  if (rows <= 0 || V <= 0 || nc <= 0 || nc > CAND_MAX || nc > V || ld < V || lp_ld < V || max_len < 0 || !(temperature > 0.f))
    return ST5_ERR_ARG;
  hipLaunchKernelGGL((beam_ctc_candidates_kernel<false, CtcScalar>), dim3(rows), dim3(bsel::THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), logits, ld, V, temperature, never, counter, max_len, lp, lp_ld, cs, nc, CtcScalar{});
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
  hipLaunchKernelGGL((ctc_prefix_score_rows_dev_kernel<false, CtcScalar>), dim3(S * beam), dim3(threads), 0,
                     reinterpret_cast<hipStream_t>(stream), x, lens, S, Tfr, V, blank, eos, beam, r_prev, tok, tok_ld,
                     counter, max_len, cs, nc, log_psi, r_new, prev, lp, lp_ld, (float)(1.0 - ctc_weight), (float)ctc_weight, CtcScalar{});
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
  hipLaunchKernelGGL((ctc_select_dev_kernel<false, CtcScalar>), dim3(S * beam), dim3(SELECT_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), lens, S, Tfr, beam, S * beam, cs, nc, log_psi, r_new, parent, tok, tok_ld, ignore,
                     sent_done, counter, max_len, state, prev, unknown, CtcScalar{});
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

// ---- the per-slot forms ----
static bool ctc_sents_shape_ok(int32_t n_slots, int32_t beam, int32_t cap) {
  return n_slots > 0 && n_slots <= 65535 && beam > 0 && beam <= 32 && cap >= 0 && (int64_t)n_slots * beam <= 0x7fffffffll;
}

extern "C" int st5_beam_ctc_candidates_sents(const float* logits, int64_t ld, int32_t n_slots, int32_t beam, int32_t V, float temperature,
                                             const uint8_t* never, const int32_t* pos, const int32_t* maxlen, const int32_t* done,
                                             int32_t cap, float* lp, int64_t lp_ld, int32_t* cs, int32_t nc, void* stream) {
  if (!logits || !never || !pos || !maxlen || !done || !lp || !cs) return ST5_ERR_ARG;
  if (!ctc_sents_shape_ok(n_slots, beam, cap) || V <= 0 || nc <= 0 || nc > CAND_MAX || nc > V || ld < V || lp_ld < V ||
      !(temperature > 0.f))
    return ST5_ERR_ARG;
  hipLaunchKernelGGL((beam_ctc_candidates_kernel<true, CtcSents>), dim3(n_slots * beam), dim3(bsel::THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), logits, ld, V, temperature, never, pos, cap, lp, lp_ld, cs, nc,
                     CtcSents{maxlen, done, nullptr, beam});
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_ctc_prefix_score_rows_sents(const float* x, const int32_t* frames, int32_t n_slots, int32_t S, int32_t V, int32_t blank,
                                               int32_t eos, int32_t beam, const float* r_prev, const int32_t* tok, int32_t tok_ld,
                                               const int32_t* pos, const int32_t* maxlen, const int32_t* done, int32_t cap,
                                               const int32_t* cs, int32_t nc, float* log_psi, float* r_new, const float* prev, float* lp,
                                               int64_t lp_ld, double ctc_weight, void* stream) {
  if (!x || !frames || !r_prev || !tok || !pos || !maxlen || !done || !cs || !log_psi || !r_new || !prev || !lp) return ST5_ERR_ARG;
  if (!ctc_sents_shape_ok(n_slots, beam, cap) || S <= 0 || V <= 0 || nc <= 0 || nc > CAND_MAX) return ST5_ERR_ARG;
  if (blank < 0 || blank >= V || eos < 0 || eos >= V || tok_ld < cap + 1 || lp_ld < V) return ST5_ERR_ARG;
  if (!(ctc_weight >= 0.0 && ctc_weight <= 1.0)) return ST5_ERR_ARG;
  const int threads = (nc + 63) / 64 * 64;
  hipLaunchKernelGGL((ctc_prefix_score_rows_dev_kernel<true, CtcSents>), dim3(n_slots * beam), dim3(threads), 0,
                     reinterpret_cast<hipStream_t>(stream), x, frames, n_slots, S, V, blank, eos, beam, r_prev, tok, tok_ld,
                     pos, cap, cs, nc, log_psi, r_new, prev, lp, lp_ld, (float)(1.0 - ctc_weight), (float)ctc_weight,
                     CtcSents{maxlen, done, nullptr, beam});
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_ctc_select_sents(const int32_t* frames, int32_t n_slots, int32_t S, int32_t beam, const int32_t* cs, int32_t nc,
                                    const float* log_psi, const float* r_new, const int32_t* parent, const int32_t* tok, int32_t tok_ld,
                                    const uint8_t* ignore, const int32_t* pos, const int32_t* maxlen, const int32_t* done,
                                    const int32_t* moved, int32_t cap, float* state, float* prev, int32_t* unknown, void* stream) {
  if (!frames || !cs || !log_psi || !r_new || !parent || !tok || !ignore || !pos || !maxlen || !done || !moved || !state || !prev ||
      !unknown)
    return ST5_ERR_ARG;
  if (!ctc_sents_shape_ok(n_slots, beam, cap) || S <= 0 || nc <= 0 || nc > CAND_MAX || tok_ld < cap + 1) return ST5_ERR_ARG;
  hipLaunchKernelGGL((ctc_select_dev_kernel<true, CtcSents>), dim3(n_slots * beam), dim3(SELECT_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), frames, n_slots, S, beam, n_slots * beam, cs, nc, log_psi, r_new, parent, tok,
                     tok_ld, ignore, done, pos, cap, state, prev, unknown, CtcSents{maxlen, nullptr, moved, beam});
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_ctc_sents_admit(const int32_t* desc, int32_t n_admit, int32_t n_slots, int32_t beam, const float* x, int32_t S, int32_t V,
                                   int32_t blank, int32_t* frames, float* state, float* prev, int32_t* unknown, void* stream) {
  if (n_admit == 0) return ST5_OK;
  if (!desc || !x || !frames || !state || !prev || !unknown) return ST5_ERR_ARG;
  if (!ctc_sents_shape_ok(n_slots, beam, 0) || n_admit < 0 || n_admit > n_slots || S <= 0 || V <= 0 || blank < 0 || blank >= V)
    return ST5_ERR_ARG;
  hipLaunchKernelGGL(ctc_sents_admit_kernel, dim3(n_admit), dim3(ADMIT_THREADS), 0, reinterpret_cast<hipStream_t>(stream), desc, n_slots,
                     beam, x, S, V, blank, frames, state, prev, unknown);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}
