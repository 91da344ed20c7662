// Index arithmetic of the per-sentence beam step and of the admission kernel of the beam-search stream (csrc/beam_step.hip:
// st5_beam_step_sents, st5_beam_reorder_sents, st5_beam_embed_sents, st5_beam_sents_admit; speecht5_amd/beam_stream.py), as inline
// functions that compile for the device AND for the host: tests/test_beam_stream_cpu.py builds this header with the host compiler
// and sweeps it.  Nothing here reads memory.
//
// A stream steps n_slots sentence slots of `beam` hypothesis rows each; slot s owns rows s*beam .. s*beam + beam - 1.  Every slot has
// its own step pos[s] and step limit maxlen[s] in device memory; cap is the largest limit the stream's buffers take, Tmax = cap + 2
// the columns of tok / score / anc, cap + 1 the columns of a record.  Whatever a kernel reads from device memory (pos, maxlen, the
// fields of an admission descriptor) goes through one of these functions before it becomes an index.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BST_HD __host__ __device__ __forceinline__
#else
#define BST_HD inline
#endif

BST_HD long long bst_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }
// a slot index read from a descriptor: outside [0, n_slots) nothing is admitted
BST_HD bool bst_slot_ok(long long slot, long long n_slots) { return slot >= 0 && slot < n_slots; }
// first hypothesis row of a slot
BST_HD long long bst_row0(long long slot, long long beam) { return slot * beam; }
// a step limit brought into [0, cap]
BST_HD int bst_maxlen(long long maxlen, long long cap) { return (int)bst_clamp(maxlen, 0, cap); }
// does a slot at `pos` with the (clamped) limit `maxlen` take a step?  Steps 0 .. maxlen run, as the scalar step's counter does.
BST_HD bool bst_step_live(long long pos, long long maxlen) { return pos >= 0 && pos <= maxlen; }
// the column the continuing rows of step `step` are written to (only below the limit), always < Tmax = cap + 2
BST_HD long long bst_next_col(long long step) { return step + 1; }
// is the sentence finished behind step `step`?
BST_HD bool bst_finished(long long n_hyp, long long beam, long long step, long long maxlen) { return n_hyp == beam || step == maxlen; }
// columns 0 .. n - 1 of the ancestry table that the reorder behind a step rewrites, for the position `pos` the step left; the step
// at the limit writes no parents, so positions past the limit (and position 0: no step has run) reorder nothing
BST_HD long long bst_reorder_cols(long long pos, long long maxlen, long long Tmax) {
  if (pos < 1 || pos > maxlen) return 0;
  return pos < Tmax ? pos : Tmax;
}
// the token column the pre-net row reads for a slot at `pos`
BST_HD int bst_embed_col(long long pos, long long Tmax) { return (int)bst_clamp(pos, 0, Tmax - 1); }
// the positional row for that column
BST_HD int bst_pos_row(long long col, long long pos_off, long long pos_rows) { return (int)bst_clamp(col + pos_off, 0, pos_rows - 1); }
// admission: encoder frames brought into [0, S]; the key-padding byte of key j (1 = excluded)
BST_HD int bst_frames(long long frames, long long S) { return (int)bst_clamp(frames, 0, S); }
BST_HD uint8_t bst_kpm_byte(long long j, long long frames) { return j >= frames ? 1 : 0; }
// element offsets of the admission's writes
BST_HD long long bst_kpm_off(long long slot, long long S, long long j) { return slot * S + j; }
BST_HD long long bst_cell_off(long long row, long long ld, long long col) { return row * ld + col; }

// ---- joint CTC / attention scoring per slot (csrc/beam_ctc.hip: st5_beam_ctc_candidates_sents, st5_ctc_prefix_score_rows_sents,
// st5_ctc_select_sents, st5_ctc_sents_admit; tests/test_beam_stream_ctc_cpu.py sweeps these).  The posterior is x [n_slots][S][V], the
// prefix states state [rows][S][2], the extensions' states r_new [rows][S][nc][2], log_psi / cs [rows][nc]; frames[s] of a slot's S
// frames are its sentence's.  Offsets of state and r_new count float2 cells.
// the slot of a hypothesis row
BST_HD long long bst_slot_of(long long row, long long beam) { return row / beam; }
// does a slot take the scoring part of a step (the CTC kernels in front of the beam step; the LM term, csrc/beam_lm.hip
// st5_beam_lm_logprobs_sents; tests/test_beam_stream_lm_cpu.py sweeps it)?  Not when it is done (finished or idle), and only at the
// steps the beam step runs.  bst_ctc_live is the name the CTC kernels know it by.
BST_HD bool bst_slot_live(long long done, long long pos, long long maxlen) { return done == 0 && bst_step_live(pos, maxlen); }
BST_HD bool bst_ctc_live(long long done, long long pos, long long maxlen) { return bst_slot_live(done, pos, maxlen); }
// does the select behind a step act on a slot?  Only where that step moved it and wrote continuing rows: the step at the limit
// writes none, and it leaves pos = maxlen + 1
BST_HD bool bst_select_live(long long moved, long long pos, long long maxlen) { return moved != 0 && pos >= 1 && pos <= maxlen; }
// a parent row read from device memory: it must lie inside the row's own slot, so no slot reads another's extensions
BST_HD bool bst_parent_ok(long long parent, long long slot, long long beam) {
  return parent >= bst_row0(slot, beam) && parent < bst_row0(slot, beam) + beam;
}
// a candidate token read from device memory
BST_HD bool bst_token_ok(long long token, long long V) { return token >= 0 && token < V; }
// element offsets: the slot's posterior, a row's prefix state, a row's extension by candidate c at frame 0 (frame f: + f * nc), a
// row's candidate cell
BST_HD long long bst_x_off(long long slot, long long S, long long V) { return slot * S * V; }
BST_HD long long bst_state_off(long long row, long long S) { return row * S; }
BST_HD long long bst_rnew_off(long long row, long long S, long long nc, long long c) { return row * S * nc + c; }
BST_HD long long bst_cand_off(long long row, long long nc, long long j) { return row * nc + j; }
