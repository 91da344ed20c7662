// Shallow fusion of a language model inside a device-stepped beam search step (SequenceGenerator(decode="device" / "graph",
// lm_model=...), speecht5_amd/beam_graph.py): what the generator does with the LM's logits between the decoder's log-probabilities and
// the rules (sequence_generator.py _generate: lprobs[:, :V_lm] += lm_weight * log_softmax(lm_logits)), for the step held in the int32
// device counter of beam_step.hip.  One launch, one workgroup per hypothesis row, step = *counter; nothing is written when step < 0 or
// step > max_len.
// st5_beam_lm_logprobs, two forms:
//   with decoder logits (no CTC in the step): lp[r][c] = (logits[r][c] / temperature - mx) - lse, the statistics (bsel::row_stats) and
//     the expression of beam_step_kernel stage 1, as st5_beam_ctc_candidates writes it; then for c < V_lm
//     lp[r][c] += w * ((x_lm[r][c] - mx_lm) - lse_lm), st5_lm_fuse_logprobs's expression.  st5_beam_step_logprobs follows.
//   in place (logits == NULL; CTC in the step): the same LM term is added into lp, which holds the CTC-mixed log-probabilities;
//     launched behind st5_ctc_prefix_score_rows_dev and in front of st5_beam_step_logprobs, the generator's order.
// The product and the sum are each rounded to fp32 on their own, as torch's `lprobs[:, :V_lm] += w * log_softmax` is.  Columns
// V_lm .. V - 1 get no LM term; -inf + (finite) stays -inf; with w = 0 the product is a zero and the sum returns lp's own bits.  The
// LM's statistics are the decoder's (bsel::row_stats at temperature 1: one wave, the row maximum in fp32, the sum of expf in fp64).
// A row is read from global memory in every pass (V is general, a row need not fit in LDS).  Plain vector loads and stores only; the
// only value read from device memory is the counter, and it only gates the launch.
// st5_beam_lm_logprobs_sents is the per-slot form (the step of a beam-search stream with an LM, speecht5_amd/beam_stream.py; index
// arithmetic: beam_stream_index.h): the same kernel body under a template flag, as csrc/beam_ctc.hip builds its _sents forms.  Row r
// belongs to slot s = r / beam and reads pos[s], maxlen[s] (clamped into [0, cap]) and done[s] where the scalar form reads one counter
// and one max_len; a slot that is done, or whose step is not live, returns before its first load and writes nothing.  The values read
// there only gate the workgroup, so the bits of a live row are the scalar form's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "beam_select.h"
#include "beam_stream_index.h"
#include "../../include/speecht5_hip.h"

namespace {

// lp + w * ((x - mx) - lse) in fp32: a product and a sum, each rounded on its own (no fused multiply-add: torch's expression has none)
__device__ __forceinline__ float lm_fuse(float lp, float w, float x, float mx, float lse) {
#pragma clang fp contract(off)
  const float term = w * ((x - mx) - lse);
  return lp + term;
}

// Where a launch takes its step from, as csrc/beam_ctc.hip does it: `counter` and `max_len` are the launch's one counter and one limit
// (X = LmScalar), or the stream's pos [n_slots] and its cap with the rest of the slot state in X = LmSents: slot s = row / beam has its
// own pos[s], maxlen[s] (clamped into [0, cap]) and done[s] (BeamStreamState).
struct LmScalar {};
struct LmSents { const int32_t* maxlen; const int32_t* done; int beam; };

template <bool SENTS, typename T, typename X>
__global__ void __launch_bounds__(bsel::THREADS)
beam_lm_logprobs_kernel(const float* __restrict__ logits, int64_t ld, int V, float temperature, const T* __restrict__ lm, int64_t lm_ld,
                        int V_lm, float w, const int32_t* __restrict__ counter, int max_len, float* __restrict__ lp, int64_t lp_ld,
                        const X sx) {
  // the gate is uniform per workgroup (one workgroup per row; the cells read are the same for every thread): false, and the
  // workgroup returns before its first load of a row
  if constexpr (SENTS) {
    const int s = (int)bst_slot_of(blockIdx.x, sx.beam);
    if (!bst_slot_live(sx.done[s], counter[s], bst_maxlen(sx.maxlen[s], max_len))) return;
  } else {
    const int step = *counter;
    if (step < 0 || step > max_len) return;
  }
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  __shared__ float s_mx, s_lse, s_mx_lm, s_lse_lm;
  const float* x = logits ? logits + (int64_t)r * ld : nullptr;
  const T* y = lm + (int64_t)r * lm_ld;
  float* out = lp + (int64_t)r * lp_ld;
  if (wave == 0 && x) {                    // one wave, as in beam_step_kernel: the same order of the reductions, the same bits
    float mx, lse;
    bsel::row_stats(x, V, temperature, lane, mx, lse);
    if (lane == 0) { s_mx = mx; s_lse = lse; }
  }
  if (wave == 1) {
    float mx, lse;
    bsel::row_stats(y, V_lm, 1.f, lane, mx, lse);
    if (lane == 0) { s_mx_lm = mx; s_lse_lm = lse; }
  }
  bsel::sync();
  const float mx_lm = s_mx_lm, lse_lm = s_lse_lm;
  if (x) {
    const float mx = s_mx, lse = s_lse;
    for (int c = tid; c < V; c += bsel::THREADS) {
      float v = (x[c] / temperature - mx) - lse;
      if (c < V_lm) v = lm_fuse(v, w, Elem<T>::to_f(y[c]), mx_lm, lse_lm);
      out[c] = v;
    }
  } else {
    for (int c = tid; c < V_lm; c += bsel::THREADS) out[c] = lm_fuse(out[c], w, Elem<T>::to_f(y[c]), mx_lm, lse_lm);
  }
}

}  // namespace

extern "C" int st5_beam_lm_logprobs(const float* logits, int64_t ld, int32_t rows, int32_t V, float temperature, const void* lm_logits,
                                    int64_t lm_ld, int32_t V_lm, float lm_weight, int lm_dtype, const int32_t* counter, int32_t max_len,
                                    float* lp, int64_t lp_ld, void* stream) {
  if (!lm_logits || !counter || !lp) return ST5_ERR_ARG;
  if (rows <= 0 || V <= 0 || V_lm <= 0 || V_lm > V || lm_ld < V_lm || lp_ld < V || max_len < 0) return ST5_ERR_ARG;
  if (logits && (ld < V || !(temperature > 0.f) || logits == lp)) return ST5_ERR_ARG;
  if (lm_dtype != ST5_F32 && lm_dtype != ST5_BF16) return ST5_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (lm_dtype == ST5_F32)
    hipLaunchKernelGGL((beam_lm_logprobs_kernel<false, float, LmScalar>), dim3(rows), dim3(bsel::THREADS), 0, st, logits, ld, V,
                       temperature, static_cast<const float*>(lm_logits), lm_ld, V_lm, lm_weight, counter, max_len, lp, lp_ld, LmScalar{});
  else
    hipLaunchKernelGGL((beam_lm_logprobs_kernel<false, bf16_t, LmScalar>), dim3(rows), dim3(bsel::THREADS), 0, st, logits, ld, V,
                       temperature, static_cast<const bf16_t*>(lm_logits), lm_ld, V_lm, lm_weight, counter, max_len, lp, lp_ld, LmScalar{});
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

// ---- the per-slot form ----
extern "C" int st5_beam_lm_logprobs_sents(const float* logits, int64_t ld, int32_t n_slots, int32_t beam, int32_t V, float temperature,
                                          const void* lm_logits, int64_t lm_ld, int32_t V_lm, float lm_weight, int lm_dtype,
                                          const int32_t* pos, const int32_t* maxlen, const int32_t* done, int32_t cap, float* lp,
                                          int64_t lp_ld, void* stream) {
  if (!lm_logits || !pos || !maxlen || !done || !lp) return ST5_ERR_ARG;
  if (n_slots <= 0 || n_slots > 65535 || beam <= 0 || beam > 32 || cap < 0) return ST5_ERR_ARG;
  if (V <= 0 || V_lm <= 0 || V_lm > V || lm_ld < V_lm || lp_ld < V) return ST5_ERR_ARG;
  if (logits && (ld < V || !(temperature > 0.f) || logits == lp)) return ST5_ERR_ARG;
  if (lm_dtype != ST5_F32 && lm_dtype != ST5_BF16) return ST5_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const LmSents sx{maxlen, done, beam};
  if (lm_dtype == ST5_F32)
    hipLaunchKernelGGL((beam_lm_logprobs_kernel<true, float, LmSents>), dim3(n_slots * beam), dim3(bsel::THREADS), 0, st, logits, ld, V,
                       temperature, static_cast<const float*>(lm_logits), lm_ld, V_lm, lm_weight, pos, cap, lp, lp_ld, sx);
  else
    hipLaunchKernelGGL((beam_lm_logprobs_kernel<true, bf16_t, LmSents>), dim3(n_slots * beam), dim3(bsel::THREADS), 0, st, logits, ld, V,
                       temperature, static_cast<const bf16_t*>(lm_logits), lm_ld, V_lm, lm_weight, pos, cap, lp, lp_ld, sx);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}
