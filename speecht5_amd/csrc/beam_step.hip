// The beam step of ASR beam search on the device (SequenceGenerator(decode="device" / "graph"), speecht5_amd/beam_graph.py): everything
// between the output projection and the next decode step, for the step index held in an int32 device counter, with no host-visible
// decision.  One workgroup per sentence; finished sentences stay in the batch (their rows keep running, their records are frozen).
//
// st5_beam_step, for step = *counter (nothing is written once step > max_len):
//   1. lprobs[r][c] = log_softmax(logits[r] / temperature)[c] in fp32 (row maximum, sum of expf in fp64 over the wave's lanes);
//   2. the rules in the generator's order: eos -inf while step < min_len, NaN -> -inf, pad -inf, unk -= unk_penalty, never[c] -> -inf,
//      at step >= max_len everything but eos -inf (optionally written out: `lprobs_out`);
//   3. the top 2 * beam of lprobs + prev over the sentence's beam * V candidates (step 0: beam row 0's V candidates), ordered by the
//      64-bit key (monotone image of the fp32 score, ~flat index): higher score first, among equal scores (-inf included, -0 = +0) the
//      lower flat index beam_row * V + token first.  The key is unique, so the order is total and there is no tie to break later.
//      Selection (beam_select.h, shared with beam_ctc.hip): MSB-first radix select on the key (8 bits a pass, one LDS histogram bin
//      per thread, stops as soon as the bucket that holds the k-th key is taken whole: after the 4 score bytes when the scores differ),
//      one gather pass, a rank sort of the 2 * beam keys.  The score of a candidate is recomputed from the logits in every pass (V is
//      general, a row need not fit in LDS);
//   4. the generator's EOS logic on the sorted candidates (one thread: 2 * beam <= 64 entries): an eos candidate among the first `beam`
//      with a finite score and a rank whose ignore flag is clear is a finished hypothesis; the first `beam` candidates that are
//      neither finished-eos nor (rank < beam and ignored) continue, then the masked ones in rank order; the new ignore flags follow;
//   5. finished hypotheses are appended to the sentence's record while it holds fewer than `beam` and the sentence is not finished:
//      tokens (without bos, closing eos) and cumulative scores are GATHERED through the ancestry table from the slot-layout histories,
//      tokens[i] = tok[anc[p][i + 1]][i + 1], positional scores are the differences of the cumulative ones; the sentence is finished
//      at `beam` hypotheses or at step == max_len, and counted once in *n_finished;
//   6. continuing row k of the sentence: tok[r][step + 1], score[r][step + 1], parent[r] (a row index of the whole launch), ignore[r];
//      the last workgroup to finish advances the counter.
// st5_beam_step_logprobs: the same kernel on log-probabilities (the CTC-mixed ones of beam_ctc.hip): stage 1 is skipped, mx = lse = 0
//   and temperature 1 leave the expression of stage 2 at x[c], bit for bit.
// st5_beam_reorder_dev: the ancestry reorder for the step the counter has just left, IN PLACE: parents lie inside the row's own
//   sentence, so the thread that owns column j of a sentence reads its `beam` entries before it writes them.
// st5_beam_embed_step: the text decoder pre-net's newest row, embed_scale * E[tok[r][counter]] + pos[counter + pos_off].
// The per-sentence forms (the step of a beam-search stream, speecht5_amd/beam_stream.py; index arithmetic: beam_stream_index.h):
// st5_beam_step_sents: the same kernel body with step = pos[s] and max_len = maxlen[s] per workgroup (a template parameter); a slot
//   whose done flag is set writes moved[s] = 0 and returns before its first load of logits; otherwise stages 1 - 6, then one thread
//   writes pos[s] + 1, the slot's pos_rows and moved[s] = 1.  No counter, no ticket: no workgroup reads another slot's position.
// st5_beam_step_sents_logprobs: st5_beam_step_sents on log-probabilities (the CTC-mixed ones of a stream with joint_ctc), as
//   st5_beam_step_logprobs is st5_beam_step on them.
// st5_beam_reorder_sents / st5_beam_embed_sents: the two launches above at the slot's own position (the reorder only where moved).
// st5_beam_sents_admit: hands finished slots to new sentences (state reset, record header emptied, key-padding bytes).
// Plain vector loads and stores only; the hand-off between the launches of a step is the kernel boundary.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "beam_select.h"
#include "beam_stream_index.h"
#include "../../include/speecht5_hip.h"

namespace {

constexpr int BS_THREADS = bsel::THREADS;
constexpr int BS_WAVES = bsel::WAVES;
constexpr int BS_MAX_BEAM = 32;
constexpr int BS_MAX_K = 2 * BS_MAX_BEAM;

using bsel::u64;
using bsel::fkey;
using bsel::unfkey;

struct BeamStepArgs {
  const float* logits; int64_t ld;
  float* lprobs; int64_t lp_ld;
  int n_sent, beam, V, Tmax;
  float temperature; int logprobs;      // logprobs: `logits` holds log-probabilities (stage 1 is skipped)
  int32_t* tok; float* score; const int32_t* anc; int64_t anc_ld;
  uint8_t* ignore; int32_t* parent;
  int32_t* rec_tok; float* rec_pos; int64_t rec_ld; float* rec_score; int32_t* rec_len;
  int32_t* n_hyp; int32_t* sent_done; int32_t* n_finished; uint32_t* ticket; int32_t* counter;
  const uint8_t* never; const float* len_div;
  int pad, unk, eos; float unk_penalty; int min_len, max_len;
};

// The per-sentence form (st5_beam_step_sents): the step and its limit are the sentence slot's own.  sent_done is the stream's `done`
// (1 = finished or idle), max_len the stream's cap (the limit's clamp); counter, n_finished and ticket are not used.
struct BeamStepSentsArgs : BeamStepArgs {
  int32_t* pos; const int32_t* maxlen; int32_t* moved; int32_t* pos_rows;
};

// one candidate's ruled log-probability (the same expression wherever it is needed: the selection passes must see the same bits)
#pragma clang fp contract(off)
__device__ __forceinline__ float bs_ruled(const BeamStepArgs& a, const float* __restrict__ x, int c, float mx, float lse, int step,
                                          int max_len) {
  float lp = (x[c] / a.temperature - mx) - lse;
  if (c == a.eos && step < a.min_len) lp = -INFINITY;
  if (lp != lp) lp = -INFINITY;
  if (c == a.pad) lp = -INFINITY;
  if (c == a.unk) lp -= a.unk_penalty;
  if (a.never[c]) lp = -INFINITY;
  if (step >= max_len && c != a.eos) lp = -INFINITY;
  return lp;
}

#pragma clang fp contract(off)
__device__ __forceinline__ u64 bs_key(const BeamStepArgs& a, int64_t row0, int b, int c, const float* s_mx, const float* s_lse,
                                      const float* s_prev, int step, int max_len) {
  float s = bs_ruled(a, a.logits + (row0 + b) * a.ld, c, s_mx[b], s_lse[b], step, max_len);
  if (step > 0) s = s + s_prev[b];
  return ((u64)fkey(s) << 32) | (uint32_t)(~(uint32_t)(b * a.V + c));
}

// SENTS = false (Args = BeamStepArgs): one step index for the launch, in *counter.  SENTS = true (Args = BeamStepSentsArgs): workgroup
// s steps slot s at pos[s] under maxlen[s]; a slot whose done flag is set, or whose position is outside 0 .. maxlen, clears moved[s]
// and touches nothing else.  No workgroup reads another slot's pos, so the hand-off to the next launch is the kernel boundary.
template <bool SENTS, typename Args>
__global__ void __launch_bounds__(BS_THREADS) beam_step_kernel(const Args a) {
  int step_, max_len_;
  if constexpr (SENTS) {
    const int s = blockIdx.x;
    max_len_ = bst_maxlen(a.maxlen[s], a.max_len);
    step_ = a.pos[s];
    if (a.sent_done[s] != 0 || !bst_step_live(step_, max_len_)) {     // (before the first load of logits)
      if (threadIdx.x == 0) a.moved[s] = 0;
      return;
    }
  } else {
    step_ = *a.counter;                          // (every workgroup reads it before the last one to finish advances it)
    max_len_ = a.max_len;
    if (step_ < 0 || step_ > max_len_) return;
  }
  const int step = step_, max_len = max_len_;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int beam = a.beam, V = a.V, K = 2 * beam, Tmax = a.Tmax;
  const int rows = a.n_sent * beam;
  const int64_t row0 = (int64_t)s * beam;

  __shared__ float s_mx[BS_MAX_BEAM], s_lse[BS_MAX_BEAM], s_prev[BS_MAX_BEAM];
  __shared__ u64 s_sorted[BS_MAX_K];
  __shared__ int s_nnew;
  __shared__ int s_fin_parent[BS_MAX_BEAM], s_fin_slot[BS_MAX_BEAM];
  __shared__ float s_fin_score[BS_MAX_BEAM];

  // ---- 1. row maximum and log-sum-exp: one wave per row in turn (log-probability input: both are zero) ----
  for (int b = wave; b < beam; b += BS_WAVES) {
    float mx = 0.f, lse = 0.f;
    if (!a.logprobs) bsel::row_stats(a.logits + (row0 + b) * a.ld, V, a.temperature, lane, mx, lse);
    if (lane == 0) {
      s_mx[b] = mx;
      s_lse[b] = lse;
      s_prev[b] = step > 0 ? a.score[(row0 + b) * Tmax + step] : 0.f;
    }
  }
  __syncthreads();

  // ---- 2. the ruled log-probabilities, on request ----
  if (a.lprobs)
    for (int b = 0; b < beam; ++b) {
      const float* x = a.logits + (row0 + b) * a.ld;
      for (int c = tid; c < V; c += BS_THREADS) a.lprobs[(row0 + b) * a.lp_ld + c] = bs_ruled(a, x, c, s_mx[b], s_lse[b], step, max_len);
    }

  // ---- 3. top 2 * beam on the unique key (beam_select.h) ----
  const int nsel = bsel::select_top<BS_MAX_K>([&](int b, int c) { return bs_key(a, row0, b, c, s_mx, s_lse, s_prev, step, max_len); },
                                              step == 0 ? 1 : beam, V, K, s_sorted);   // (= K: the limits guarantee V > 2 * beam)

  // ---- 4. - 6. EOS logic, record bookkeeping and the continuing rows: 2 * beam entries, one thread ----
  if (tid == 0) {
    const bool done = SENTS ? false : a.sent_done[s] != 0;      // (a done slot of the per-sentence form has returned above)
    int nh = a.n_hyp[s], nnew = 0;
    u64 masked = 0;
    for (int i = 0; i < nsel; ++i) {
      const u64 key = s_sorted[i];
      const float sc = unfkey((uint32_t)(key >> 32));
      const uint32_t f = ~(uint32_t)key;
      const bool fin = (int)(f % (uint32_t)V) == a.eos && sc != -INFINITY;
      bool m = fin;
      if (i < beam) {
        const bool ign = a.ignore[row0 + i] != 0;
        if (fin && !ign && !done && nh < beam) {
          s_fin_parent[nnew] = (int)(f / (uint32_t)V);
          s_fin_score[nnew] = sc;
          s_fin_slot[nnew] = nh;
          ++nh;
          ++nnew;
        }
        m = ign || fin;
      }
      if (m) masked |= (u64)1 << i;
    }
    s_nnew = nnew;
    if (!done) {
      a.n_hyp[s] = nh;
      if (nh == beam || step == max_len) {        // (= bst_finished of beam_stream_index.h)
        a.sent_done[s] = 1;
        if constexpr (!SENTS) atomicAdd(a.n_finished, 1);
      }
    }
    if (step < max_len) {
      int k = 0;
      for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < nsel && k < beam; ++i) {
          const bool m = (masked >> i) & 1;
          if (m != (pass == 1)) continue;
          const u64 key = s_sorted[i];
          const uint32_t f = ~(uint32_t)key;
          const int64_t r = row0 + k;
          a.tok[r * Tmax + step + 1] = (int32_t)(f % (uint32_t)V);
          a.score[r * Tmax + step + 1] = unfkey((uint32_t)(key >> 32));
          a.parent[r] = (int32_t)(row0 + f / (uint32_t)V);
          a.ignore[r] = m ? 1 : 0;
          ++k;
        }
    }
  }
  __syncthreads();

  // ---- 5. the finished hypotheses' records: a parallel gather through the ancestry table ----
  const int nnew = s_nnew;
  for (int h = 0; h < nnew; ++h) {
    const int64_t p = row0 + s_fin_parent[h];
    const float fs = s_fin_score[h];
    const int64_t rec = (row0 + s_fin_slot[h]) * a.rec_ld;
    for (int i = tid; i <= step; i += BS_THREADS) {
      int32_t t = a.eos;
      float ci = fs, cp = 0.f;
      if (i < step) {
        const int32_t ar = a.anc[p * a.anc_ld + i + 1];
        const bool ok = ar >= 0 && ar < rows;      // (a broken ancestry entry shows up in the record, it is never dereferenced)
        t = ok ? a.tok[(int64_t)ar * Tmax + i + 1] : -1;
        ci = ok ? a.score[(int64_t)ar * Tmax + i + 1] : NAN;
      }
      if (i > 0) {
        const int32_t ar = a.anc[p * a.anc_ld + i];
        cp = (ar >= 0 && ar < rows) ? a.score[(int64_t)ar * Tmax + i] : NAN;
      }
      a.rec_tok[rec + i] = t;
      a.rec_pos[rec + i] = i > 0 ? ci - cp : ci;
    }
    if (tid == 0) {
      a.rec_score[row0 + s_fin_slot[h]] = a.len_div ? fs / a.len_div[step] : fs;
      a.rec_len[row0 + s_fin_slot[h]] = step + 1;
    }
  }

  // ---- the last workgroup to get here advances the counter; per sentence: the slot's own position, its rows' copy of it, moved ----
  __syncthreads();
  if (tid == 0) {
    if constexpr (SENTS) {
      const int32_t next = (int32_t)bst_next_col(step);
      a.pos[s] = next;
      for (int b = 0; b < beam; ++b) a.pos_rows[row0 + b] = next;
      a.moved[s] = 1;
    } else {
      __threadfence();
      const unsigned t = atomicAdd(a.ticket, 1u);
      if (t == gridDim.x - 1) {
        *a.ticket = 0;
        *a.counter = step + 1;
      }
    }
  }
}

// grid (ceil(Tmax / 256), n_sent): thread = column j of one sentence.  t = *counter positions are written; the step that wrote the
// parents is t - 1, and it wrote none at or past max_len.  SENTS (X = BeamReorderSents): sentence slot blockIdx.y is reordered for
// t = counter[slot] (the slot's pos) under its own limit, max_len being the stream's cap, and only where the step moved the slot.
struct BeamReorderScalar {};
struct BeamReorderSents { const int32_t* maxlen; const int32_t* moved; };

template <bool SENTS, typename X>
__global__ void __launch_bounds__(256) beam_reorder_dev_kernel(int32_t* __restrict__ anc, int64_t anc_ld, const int32_t* __restrict__ parent,
                                                             int beam, int Tmax, const int32_t* __restrict__ counter, int max_len, const X x) {
  int t_;
  if constexpr (SENTS) {
    const int s = blockIdx.y;
    if (x.moved[s] == 0) return;
    t_ = (int)bst_reorder_cols(counter[s], bst_maxlen(x.maxlen[s], max_len), Tmax);
    if (t_ < 1) return;
  } else {
    t_ = *counter;
    if (t_ < 1 || t_ > max_len) return;
  }
  const int t = t_;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= t || j >= Tmax) return;
  const int64_t row0 = (int64_t)blockIdx.y * beam;
  int32_t v[BS_MAX_BEAM];
#pragma unroll
  for (int b = 0; b < BS_MAX_BEAM; ++b) {
    v[b] = -1;
    if (b < beam) {
      const int64_t pl = (int64_t)parent[row0 + b] - row0;
      if (pl >= 0 && pl < beam) v[b] = anc[(row0 + pl) * anc_ld + j];
    }
  }
#pragma unroll
  for (int b = 0; b < BS_MAX_BEAM; ++b)
    if (b < beam) anc[(row0 + b) * anc_ld + j] = v[b];
}

// one wave per row: the arithmetic of embed_rows_kernel (elementwise.hip) at position t + pos_off (shared by both forms)
template <typename T>
__device__ __forceinline__ void beam_embed_row(const float* __restrict__ table, int V, const int32_t* __restrict__ tok, int Tmax, int t,
                                               const float* __restrict__ pos, int pos_rows, int pos_off, float emb_scale, T* __restrict__ y,
                                               int64_t y_ld, int row, int cols) {
  t = t < 0 ? 0 : (t > Tmax - 1 ? Tmax - 1 : t);
  int pr = t + pos_off;
  pr = pr < 0 ? 0 : (pr > pos_rows - 1 ? pos_rows - 1 : pr);
  const int32_t id = tok[(int64_t)row * Tmax + t];
  const bool ok = id >= 0 && id < V;             // (a broken token shows up as NaN, it is never dereferenced)
  const float* trow = table + (int64_t)(ok ? id : 0) * cols;
  const float* prow = pos + (int64_t)pr * cols;
  for (int c = threadIdx.x & 63; c < cols; c += 64) {
    float v = emb_scale * trow[c];
    v = fmaf(1.f, prow[c], v);
    y[(int64_t)row * y_ld + c] = Elem<T>::from_f(ok ? v : NAN);
  }
}

// grid (ceil(rows / 4)): position counter + pos_off for every row
template <typename T>
__global__ void __launch_bounds__(256) beam_embed_step_kernel(const float* __restrict__ table, int V, const int32_t* __restrict__ tok, int Tmax,
                                                            const int32_t* __restrict__ counter, const float* __restrict__ pos, int pos_rows,
                                                            int pos_off, float emb_scale, T* __restrict__ y, int64_t y_ld, int rows, int cols) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  beam_embed_row<T>(table, V, tok, Tmax, *counter, pos, pos_rows, pos_off, emb_scale, y, y_ld, row, cols);
}

// the same grid, per sentence: row r at position spos[r / beam] + pos_off (rows = n_slots * beam)
template <typename T>
__global__ void __launch_bounds__(256) beam_embed_sents_kernel(const float* __restrict__ table, int V, const int32_t* __restrict__ tok, int Tmax,
                                                             const int32_t* __restrict__ spos, int beam, const float* __restrict__ pos,
                                                             int pos_rows, int pos_off, float emb_scale, T* __restrict__ y, int64_t y_ld,
                                                             int rows, int cols) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  beam_embed_row<T>(table, V, tok, Tmax, spos[row / beam], pos, pos_rows, pos_off, emb_scale, y, y_ld, row, cols);
}

// grid (n_admit): workgroup i hands slot desc[i][0] to a new sentence with the step limit desc[i][1], desc[i][2] encoder frames and
// the first token desc[i][3].  A slot index outside [0, n_slots) admits nothing; nothing of another slot is written.
__global__ void __launch_bounds__(256) beam_sents_admit_kernel(const int32_t* __restrict__ desc, int n_slots, int beam, int cap, int Tmax,
                                                             int32_t* __restrict__ tok, float* __restrict__ score, int32_t* __restrict__ anc,
                                                             int64_t anc_ld, uint8_t* __restrict__ ignore, int32_t* __restrict__ n_hyp,
                                                             int32_t* __restrict__ rec_len, int32_t* __restrict__ pos,
                                                             int32_t* __restrict__ pos_rows, int32_t* __restrict__ maxlen,
                                                             int32_t* __restrict__ done, uint8_t* __restrict__ kpm, int S) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int slot = desc[4 * i];
  if (!bst_slot_ok(slot, n_slots)) return;
  const int ml = bst_maxlen(desc[4 * i + 1], cap);
  const int frames = bst_frames(desc[4 * i + 2], S);
  const int32_t bos = desc[4 * i + 3];          // (stored as it is: st5_beam_embed_sents range-checks every token it reads)
  const int64_t row0 = bst_row0(slot, beam);
  for (int e = tid; e < beam * Tmax; e += 256) {
    const int b = e / Tmax, j = e % Tmax;
    anc[bst_cell_off(row0 + b, anc_ld, j)] = (int32_t)(row0 + b);
  }
  for (int b = tid; b < beam; b += 256) {
    tok[bst_cell_off(row0 + b, Tmax, 0)] = bos;
    score[bst_cell_off(row0 + b, Tmax, 0)] = 0.f;
    ignore[row0 + b] = 0;
    rec_len[row0 + b] = 0;
    pos_rows[row0 + b] = 0;
  }
  for (int j = tid; j < S; j += 256) kpm[bst_kpm_off(slot, S, j)] = bst_kpm_byte(j, frames);
  if (tid == 0) {
    n_hyp[slot] = 0;
    pos[slot] = 0;
    maxlen[slot] = ml;
    done[slot] = 0;
  }
}

}  // namespace

static int beam_step_launch(int logprobs, const float* logits, int64_t ld, float* lprobs_out, int64_t lp_ld, int32_t n_sent, int32_t beam,
                            int32_t V, float temperature, int32_t* tok, float* score, const int32_t* anc, int64_t anc_ld, int32_t Tmax,
                            uint8_t* ignore, int32_t* parent, int32_t* rec_tok, float* rec_pos, int64_t rec_ld, float* rec_score,
                            int32_t* rec_len, int32_t* n_hyp, int32_t* sent_done, int32_t* n_finished, uint32_t* ticket, int32_t* counter,
                            const uint8_t* never, const float* len_div, int32_t pad, int32_t unk, int32_t eos, float unk_penalty,
                            int32_t min_len, int32_t max_len, void* stream) {
  if (!logits || !tok || !score || !anc || !ignore || !parent || !rec_tok || !rec_pos || !rec_score || !rec_len || !n_hyp || !sent_done ||
      !n_finished || !ticket || !counter || !never)
    return ST5_ERR_ARG;
  if (n_sent <= 0 || n_sent > 65535 || beam <= 0 || beam > BS_MAX_BEAM || V <= 0 || V - 1 < 2 * beam) return ST5_ERR_ARG;
  if ((int64_t)beam * V > 0x7fffffffll || (int64_t)n_sent * beam > 0x7fffffffll) return ST5_ERR_ARG;
  if (ld < V || (lprobs_out && lp_ld < V) || !(temperature > 0.f)) return ST5_ERR_ARG;
  if (max_len < 0 || min_len < 0 || Tmax < max_len + 1 || anc_ld < Tmax || rec_ld < max_len + 1) return ST5_ERR_ARG;
  if (eos < 0 || eos >= V) return ST5_ERR_ARG;
  BeamStepArgs a;
  a.logits = logits; a.ld = ld; a.lprobs = lprobs_out; a.lp_ld = lp_ld;
  a.n_sent = n_sent; a.beam = beam; a.V = V; a.Tmax = Tmax; a.temperature = temperature; a.logprobs = logprobs;
  a.tok = tok; a.score = score; a.anc = anc; a.anc_ld = anc_ld; a.ignore = ignore; a.parent = parent;
  a.rec_tok = rec_tok; a.rec_pos = rec_pos; a.rec_ld = rec_ld; a.rec_score = rec_score; a.rec_len = rec_len;
  a.n_hyp = n_hyp; a.sent_done = sent_done; a.n_finished = n_finished; a.ticket = ticket; a.counter = counter;
  a.never = never; a.len_div = len_div;
  a.pad = pad; a.unk = unk; a.eos = eos; a.unk_penalty = unk_penalty; a.min_len = min_len; a.max_len = max_len;
  hipLaunchKernelGGL((beam_step_kernel<false, BeamStepArgs>), dim3(n_sent), dim3(BS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

static int beam_step_sents_launch(int logprobs, const float* logits, int64_t ld, float* lprobs_out, int64_t lp_ld, int32_t n_slots,
                                  int32_t beam, int32_t V, float temperature, int32_t* tok, float* score, const int32_t* anc, int64_t anc_ld,
                                  int32_t Tmax, uint8_t* ignore, int32_t* parent, int32_t* rec_tok, float* rec_pos, int64_t rec_ld,
                                  float* rec_score, int32_t* rec_len, int32_t* n_hyp, int32_t* pos, const int32_t* maxlen, int32_t* done,
                                  int32_t* moved, int32_t* pos_rows, const uint8_t* never, const float* len_div, int32_t pad, int32_t unk,
                                  int32_t eos, float unk_penalty, int32_t min_len, int32_t cap, void* stream) {
  if (!logits || !tok || !score || !anc || !ignore || !parent || !rec_tok || !rec_pos || !rec_score || !rec_len || !n_hyp || !pos ||
      !maxlen || !done || !moved || !pos_rows || !never)
    return ST5_ERR_ARG;
  if (n_slots <= 0 || n_slots > 65535 || beam <= 0 || beam > BS_MAX_BEAM || V <= 0 || V - 1 < 2 * beam) return ST5_ERR_ARG;
  if ((int64_t)beam * V > 0x7fffffffll || (int64_t)n_slots * beam > 0x7fffffffll) return ST5_ERR_ARG;
  if (ld < V || (lprobs_out && lp_ld < V) || !(temperature > 0.f)) return ST5_ERR_ARG;
  if (cap < 0 || min_len < 0 || Tmax < cap + 2 || anc_ld < Tmax || rec_ld < cap + 1) return ST5_ERR_ARG;
  if (eos < 0 || eos >= V) return ST5_ERR_ARG;
  BeamStepSentsArgs a;
  a.logits = logits; a.ld = ld; a.lprobs = lprobs_out; a.lp_ld = lp_ld;
  a.n_sent = n_slots; a.beam = beam; a.V = V; a.Tmax = Tmax; a.temperature = temperature; a.logprobs = logprobs;
  a.tok = tok; a.score = score; a.anc = anc; a.anc_ld = anc_ld; a.ignore = ignore; a.parent = parent;
  a.rec_tok = rec_tok; a.rec_pos = rec_pos; a.rec_ld = rec_ld; a.rec_score = rec_score; a.rec_len = rec_len;
  a.n_hyp = n_hyp; a.sent_done = done; a.n_finished = nullptr; a.ticket = nullptr; a.counter = nullptr;
  a.never = never; a.len_div = len_div;
  a.pad = pad; a.unk = unk; a.eos = eos; a.unk_penalty = unk_penalty; a.min_len = min_len; a.max_len = cap;
  a.pos = pos; a.maxlen = maxlen; a.moved = moved; a.pos_rows = pos_rows;
  hipLaunchKernelGGL((beam_step_kernel<true, BeamStepSentsArgs>), dim3(n_slots), dim3(BS_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     a);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_beam_step_sents(const float* logits, int64_t ld, float* lprobs_out, int64_t lp_ld, int32_t n_slots, int32_t beam, int32_t V,
                                   float temperature, int32_t* tok, float* score, const int32_t* anc, int64_t anc_ld, int32_t Tmax,
                                   uint8_t* ignore, int32_t* parent, int32_t* rec_tok, float* rec_pos, int64_t rec_ld, float* rec_score,
                                   int32_t* rec_len, int32_t* n_hyp, int32_t* pos, const int32_t* maxlen, int32_t* done, int32_t* moved,
                                   int32_t* pos_rows, const uint8_t* never, const float* len_div, int32_t pad, int32_t unk, int32_t eos,
                                   float unk_penalty, int32_t min_len, int32_t cap, void* stream) {
  return beam_step_sents_launch(0, logits, ld, lprobs_out, lp_ld, n_slots, beam, V, temperature, tok, score, anc, anc_ld, Tmax, ignore, parent,
                                rec_tok, rec_pos, rec_ld, rec_score, rec_len, n_hyp, pos, maxlen, done, moved, pos_rows, never, len_div, pad,
                                unk, eos, unk_penalty, min_len, cap, stream);
}

extern "C" int st5_beam_step_sents_logprobs(const float* lp, int64_t ld, float* lprobs_out, int64_t lp_ld, int32_t n_slots, int32_t beam,
                                            int32_t V, int32_t* tok, float* score, const int32_t* anc, int64_t anc_ld, int32_t Tmax,
                                            uint8_t* ignore, int32_t* parent, int32_t* rec_tok, float* rec_pos, int64_t rec_ld,
                                            float* rec_score, int32_t* rec_len, int32_t* n_hyp, int32_t* pos, const int32_t* maxlen,
                                            int32_t* done, int32_t* moved, int32_t* pos_rows, const uint8_t* never, const float* len_div,
                                            int32_t pad, int32_t unk, int32_t eos, float unk_penalty, int32_t min_len, int32_t cap,
                                            void* stream) {
  return beam_step_sents_launch(1, lp, ld, lprobs_out, lp_ld, n_slots, beam, V, 1.f, tok, score, anc, anc_ld, Tmax, ignore, parent, rec_tok,
                                rec_pos, rec_ld, rec_score, rec_len, n_hyp, pos, maxlen, done, moved, pos_rows, never, len_div, pad, unk, eos,
                                unk_penalty, min_len, cap, stream);
}

extern "C" int st5_beam_reorder_sents(int32_t* anc, int64_t anc_ld, const int32_t* parent, int32_t n_slots, int32_t beam, int32_t Tmax,
                                      const int32_t* pos, const int32_t* maxlen, const int32_t* moved, int32_t cap, void* stream) {
  if (!anc || !parent || !pos || !maxlen || !moved) return ST5_ERR_ARG;
  if (n_slots <= 0 || n_slots > 65535 || beam <= 0 || beam > BS_MAX_BEAM || Tmax <= 0 || anc_ld < Tmax || cap < 0 || Tmax < cap + 2)
    return ST5_ERR_ARG;
  hipLaunchKernelGGL((beam_reorder_dev_kernel<true, BeamReorderSents>), dim3((Tmax + 255) / 256, n_slots), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), anc, anc_ld, parent, beam, Tmax, pos, cap, BeamReorderSents{maxlen, moved});
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_beam_embed_sents(const float* table, int32_t V, const int32_t* tok, int32_t Tmax, const int32_t* spos, int32_t n_slots,
                                    int32_t beam, const float* pos, int32_t pos_rows, int32_t pos_off, float emb_scale, void* y, int64_t y_ld,
                                    int32_t cols, int dtype, void* stream) {
  if (!table || !tok || !spos || !pos || !y) return ST5_ERR_ARG;
  if (V <= 0 || Tmax <= 0 || pos_rows <= 0 || n_slots <= 0 || beam <= 0 || beam > BS_MAX_BEAM || cols <= 0 || y_ld < cols) return ST5_ERR_ARG;
  if ((int64_t)n_slots * beam > 0x7fffffffll) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rows = n_slots * beam;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == ST5_F32)
    hipLaunchKernelGGL(beam_embed_sents_kernel<float>, grid, dim3(256), 0, st, table, V, tok, Tmax, spos, beam, pos, pos_rows, pos_off,
                       emb_scale, static_cast<float*>(y), y_ld, rows, cols);
  else
    hipLaunchKernelGGL(beam_embed_sents_kernel<bf16_t>, grid, dim3(256), 0, st, table, V, tok, Tmax, spos, beam, pos, pos_rows, pos_off,
                       emb_scale, static_cast<bf16_t*>(y), y_ld, rows, cols);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_beam_sents_admit(const int32_t* desc, int32_t n_admit, int32_t n_slots, int32_t beam, int32_t cap, int32_t Tmax, int32_t* tok,
                                    float* score, int32_t* anc, int64_t anc_ld, uint8_t* ignore, int32_t* n_hyp, int32_t* rec_len, int32_t* pos,
                                    int32_t* pos_rows, int32_t* maxlen, int32_t* done, uint8_t* kpm, int32_t S, void* stream) {
  if (n_admit == 0) return ST5_OK;
  if (!desc || !tok || !score || !anc || !ignore || !n_hyp || !rec_len || !pos || !pos_rows || !maxlen || !done || !kpm) return ST5_ERR_ARG;
  if (n_slots <= 0 || n_slots > 65535 || n_admit < 0 || n_admit > n_slots || beam <= 0 || beam > BS_MAX_BEAM) return ST5_ERR_ARG;
  if (cap < 0 || Tmax < cap + 2 || anc_ld < Tmax || S <= 0 || (int64_t)n_slots * beam > 0x7fffffffll) return ST5_ERR_ARG;
  hipLaunchKernelGGL(beam_sents_admit_kernel, dim3(n_admit), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), desc, n_slots, beam, cap,
                     Tmax, tok, score, anc, anc_ld, ignore, n_hyp, rec_len, pos, pos_rows, maxlen, done, kpm, S);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_beam_step(const float* logits, int64_t ld, float* lprobs_out, int64_t lp_ld, int32_t n_sent, int32_t beam, int32_t V,
                             float temperature, int32_t* tok, float* score, const int32_t* anc, int64_t anc_ld, int32_t Tmax,
                             uint8_t* ignore, int32_t* parent, int32_t* rec_tok, float* rec_pos, int64_t rec_ld, float* rec_score,
                             int32_t* rec_len, int32_t* n_hyp, int32_t* sent_done, int32_t* n_finished, uint32_t* ticket, int32_t* counter,
                             const uint8_t* never, const float* len_div, int32_t pad, int32_t unk, int32_t eos, float unk_penalty,
                             int32_t min_len, int32_t max_len, void* stream) {
  return beam_step_launch(0, logits, ld, lprobs_out, lp_ld, n_sent, beam, V, temperature, tok, score, anc, anc_ld, Tmax, ignore, parent,
                          rec_tok, rec_pos, rec_ld, rec_score, rec_len, n_hyp, sent_done, n_finished, ticket, counter, never, len_div, pad,
                          unk, eos, unk_penalty, min_len, max_len, stream);
}

extern "C" int st5_beam_step_logprobs(const float* lp, int64_t ld, float* lprobs_out, int64_t lp_ld, int32_t n_sent, int32_t beam, int32_t V,
                                      int32_t* tok, float* score, const int32_t* anc, int64_t anc_ld, int32_t Tmax, uint8_t* ignore,
                                      int32_t* parent, int32_t* rec_tok, float* rec_pos, int64_t rec_ld, float* rec_score, int32_t* rec_len,
                                      int32_t* n_hyp, int32_t* sent_done, int32_t* n_finished, uint32_t* ticket, int32_t* counter,
                                      const uint8_t* never, const float* len_div, int32_t pad, int32_t unk, int32_t eos, float unk_penalty,
                                      int32_t min_len, int32_t max_len, void* stream) {
  return beam_step_launch(1, lp, ld, lprobs_out, lp_ld, n_sent, beam, V, 1.f, tok, score, anc, anc_ld, Tmax, ignore, parent, rec_tok,
                          rec_pos, rec_ld, rec_score, rec_len, n_hyp, sent_done, n_finished, ticket, counter, never, len_div, pad, unk, eos,
                          unk_penalty, min_len, max_len, stream);
}

extern "C" int st5_beam_reorder_dev(int32_t* anc, int64_t anc_ld, const int32_t* parent, int32_t n_sent, int32_t beam, int32_t Tmax,
                                    const int32_t* counter, int32_t max_len, void* stream) {
  if (!anc || !parent || !counter) return ST5_ERR_ARG;
  if (n_sent <= 0 || n_sent > 65535 || beam <= 0 || beam > BS_MAX_BEAM || Tmax <= 0 || anc_ld < Tmax || max_len < 0 || Tmax < max_len + 1)
    return ST5_ERR_ARG;
  hipLaunchKernelGGL((beam_reorder_dev_kernel<false, BeamReorderScalar>), dim3((Tmax + 255) / 256, n_sent), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), anc, anc_ld, parent, beam, Tmax, counter, max_len, BeamReorderScalar{});
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}

extern "C" int st5_beam_embed_step(const float* table, int32_t V, const int32_t* tok, int32_t Tmax, const int32_t* counter, const float* pos,
                                   int32_t pos_rows, int32_t pos_off, float emb_scale, void* y, int64_t y_ld, int32_t rows, int32_t cols,
                                   int dtype, void* stream) {
  if (!table || !tok || !counter || !pos || !y) return ST5_ERR_ARG;
  if (V <= 0 || Tmax <= 0 || pos_rows <= 0 || rows <= 0 || cols <= 0 || y_ld < cols) return ST5_ERR_ARG;
  if (dtype != ST5_F32 && dtype != ST5_BF16) return ST5_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == ST5_F32)
    hipLaunchKernelGGL(beam_embed_step_kernel<float>, grid, dim3(256), 0, st, table, V, tok, Tmax, counter, pos, pos_rows, pos_off, emb_scale,
                       static_cast<float*>(y), y_ld, rows, cols);
  else
    hipLaunchKernelGGL(beam_embed_step_kernel<bf16_t>, grid, dim3(256), 0, st, table, V, tok, Tmax, counter, pos, pos_rows, pos_off, emb_scale,
                       static_cast<bf16_t*>(y), y_ld, rows, cols);
  return hipGetLastError() == hipSuccess ? ST5_OK : ST5_ERR_LAUNCH;
}
