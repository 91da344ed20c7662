/*
 * libspeecht5_hip.so -- C ABI of the MI355X (gfx950) SpeechT5 forward/backward hot path.
 *
 * The reference (microsoft/SpeechT5) has no FFI: its hot path is PyTorch op call sites inside
 * SpeechT5/speecht5/models/modules/[module].py.  Each entry point below replaces
 * the torch op(s) at the cited reference call site; INTEGRATION.md shows the ctypes stub that a
 * reference maintainer would add.  Conventions:
 *   - plain pointers + sizes, caller-owned device buffers, no torch types;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it;
 *   - `dtype` is ST5_F32 (0) or ST5_BF16 (1): the element type of activations/weights;
 *     statistics, softmax, accumulators, biases, LayerNorm affine params and weight gradients are fp32;
 *   - return value 0 = ok, non-zero = ST5_ERR_* (argument / alignment / launch error);
 *   - threading / devices: the library is built for ONE process per GPU driven by ONE host thread (the reference's
 *     execution model).  It keeps process-global mutable state -- the stream-fork event ring, the
 *     A/B switches (st5_gemm_set_*, st5_layernorm_set_max_blocks) and tables of PER-STREAM state: the deferred split-K
 *     queue with its slab arena (st5_gemm_defer_splitk / _flush_splitk; an arena is hipFree'd and re-allocated when it
 *     must grow, which synchronises the device), the split-K slab workspaces, the deferred LayerNorm reductions
 *     (st5_layernorm_defer / _flush) and the workspace of the ordered row scatter.  One host thread may therefore keep
 *     several streams busy at once (the two micro-batches of an update side by side).  Table sizes: 32 streams with
 *     deferred LayerNorm reductions and 32 with deferred split-K reductions (a 33rd, e.g. in a test session that keeps
 *     creating streams, restarts the table after a device synchronisation, provided nothing is queued on any state -- a
 *     state is never handed from one live stream to another); 8 with split-K slab workspaces (taken over after a device
 *     synchronisation).  A flush only folds what was
 *     queued on the stream it is given.  Calling the library from two host threads, or for
 *     two devices from one process, is NOT supported.
 */
#ifndef SPEECHT5_HIP_H
#define SPEECHT5_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ST5_F32 0
#define ST5_BF16 1

#define ST5_ACT_NONE 0
#define ST5_ACT_GELU 1
#define ST5_ACT_RELU 2
#define ST5_ACT_TANH 3
#define ST5_ACT_LRELU_01 4  /* LeakyReLU(0.1), HiFi-GAN */
#define ST5_ACT_LRELU_001 5 /* LeakyReLU(0.01) */

/* gemm flags */
#define ST5_GEMM_A_KSTRIDED 1  /* A(i,k) stored k-outer (i contiguous): "transposed" operand      */
#define ST5_GEMM_B_KSTRIDED 2  /* B(j,k) stored k-outer (j contiguous)                            */
#define ST5_GEMM_OUT_F32 4     /* C / R are fp32 regardless of dtype (weight gradients)           */
#define ST5_GEMM_DACT 8        /* multiply result by act'(P) (P = saved pre-activation, C layout) */
#define ST5_GEMM_DEFERRABLE 16 /* C is not read before st5_gemm_flush_splitk: a split-K reduction may be queued (st5_gemm_defer_splitk) */

/* Generalised operand addressing (elements):
 *   off(outer, inner) = (rpb ? (outer / rpb) * bstride + (outer % rpb) * ld : outer * ld)
 *                     + (seg ? (inner / seg) * seg_stride + inner % seg : inner)
 *                     + (z / zdiv) * zs0 + (z % zdiv) * zs1            (z = batch index)
 * K-major operand: outer = row (i or j), inner = k.  K-strided operand: outer = k, inner = row.
 * This one descriptor covers nn.Linear fwd/dgrad/wgrad, strided / grouped conv1d as implicit GEMM
 * on channels-last activations (overlapping rows: ld = stride*C, inner spans k*C), and the
 * per-(batch,head) attention matmuls. */
typedef struct st5_operand {
  const void* ptr;
  int64_t ld;
  int32_t rpb;
  int32_t seg;
  int64_t bstride;
  int64_t seg_stride;
  int64_t zs0, zs1;
} st5_operand;

typedef struct st5_gemm_params {
  st5_operand A;    /* [M x K] */
  st5_operand B;    /* [N x K] (nn.Linear weight layout when K-major) */
  st5_operand C;    /* [M x N] output; outer = row, inner = col */
  st5_operand R;    /* optional residual added to the output (ptr may be NULL), C layout */
  st5_operand P;    /* optional pre-activation for ST5_GEMM_DACT, C layout */
  st5_operand Cpre; /* optional second output receiving the pre-activation value, C layout */
  const float* bias; /* optional fp32 [N] (+ z * bias_zs) */
  int64_t bias_zs;
  int32_t M, N, K;
  int32_t batch, zdiv;
  int32_t act;      /* ST5_ACT_* applied after bias */
  int32_t flags;
  float alpha;      /* scales A*B before bias */
  float beta;       /* C = result + beta * C_old (0 => C_old not read) */
  float dropout_p;  /* dropout applied last (after act, before residual); 0 => off */
  uint64_t seed;    /* dropout RNG seed; element counter = z*M*N + row*N + col, for every N and every C layout (N % 8 != 0 included:
                     * the epilogue then evaluates the rule element by element); pinned by tests/test_gemm_fp64_gpu.py */
  float* asum;      /* optional fp32 [M] (batch == 1): asum[m] += sum_k A(m, k).  With A = dY^T this is the bias gradient,
                     * computed by the weight-gradient GEMM itself (one extra MFMA column in the first column of tiles)
                     * instead of a separate reduction over dY (autograd of F.linear: grad_bias = dY.sum(0)). */
  const float* gate; /* optional LayerDrop layer gate: one float in device memory (the `keep` of st5_layernorm_gated_fwd).  When *gate == 0
                      * every block of the launch exits before it reads or writes anything: C, Cpre and asum stay as they are (a dropped
                      * layer's activations are never read; its weight / bias gradient accumulators would only receive exact zeros).
                      * A split-K reduction, immediate or deferred, honours it too.  NULL or *gate != 0: no effect, bit for bit.
                      * In st5_gemm_tn_group the gate is per problem.  Ignored by the MX-fp8 entry points. */
} st5_gemm_params;

/* Generic MFMA GEMM: C = drop(act(alpha * A.B^T + bias)) [* act'(P)] + R + beta*C.
 * Replaces F.linear at multihead_attention.py:213-231,397; transformer_layer.py:127-131,385-389;
 * speech_encoder_prenet.py:177; F.conv1d at speech_encoder_prenet.py:300 (layers 1..6) and :107
 * (pos_conv); torch.bmm at multihead_attention.py:340,389; and their autograd backward passes. */
int st5_gemm(const st5_gemm_params* p, int dtype, void* stream);
/* 1 (default): plain NT GEMMs use the LDS-DMA pipelined kernel; 0: always the register-staged kernel (A/B testing).
 * The same kernels take B k-strided ("NN": bf16, batch 1, no asum, A not k-strided, B without row split / segments and 16-byte aligned with a
 * leading dimension that is a multiple of 8, N % 8 == 0, K % 64 == 0, K >= 128) -- same bits as the NT call on a transposed copy of B. */
/* Stream ordering for the host side (no torch types): everything enqueued on `to` after this call runs after everything
 * enqueued on `from` before it.  Used to run the weight-gradient GEMMs of a backward pass (off the critical path: only the
 * optimizer / gradient all-reduce needs them) on a second stream beside the data-gradient chain. */
int st5_stream_fork(void* from_stream, void* to_stream);
int st5_gemm_set_glds(int enabled);
/* NT block tile: 0 = chosen per problem (default), 1 = 128x128 always, 2 = first 256x256 kernel always, 3 / 4 = phased 256x256 kernel always
 * with / without the half-phase stagger, 5 = 64x128 kernel always (A/B measurements only). */
int st5_gemm_set_nt_tile(int mode);
/* (mode 5 = the 64x128 kernel always.)  bf16 NT GEMMs of at most `tiles` tiles of 128x128 (x batch) run on 64x128 tiles, three blocks per CU
 * (round 6: the transformer's Linear GEMMs at 8 utterances per GPU -- modules/transformer_layer.py:127-131, multihead_attention.py:213-231 --
 * are 0.25-3 rounds of 128x128 tiles); 0 = never.  Results are bit-identical for every choice. */
int st5_gemm_set_m64_max_tiles(int tiles);
/* (A/B) bf16 NT GEMMs of at least `tiles` tiles of 256x256 with at least `nk` k-tiles of 64 also run on the phased 256x256 kernel (the
 * N = 768 long-reduction shapes: one block on 96 CUs instead of 384 tiles of 128x128 on all of them); tiles = 0: off (default). */
int st5_gemm_set_nt_longk(int tiles, int nk);
/* Block count the split-K choice of the fp32-output (weight-gradient) GEMMs aims for; default 384 (1.5 per CU). */
int st5_gemm_set_splitk_target(int blocks);
/* Weight-gradient (TN form, no row split / segments) GEMMs: 0 (default) = always the 128x128 LDS-DMA kernel; 1 = phased 256x256 kernel with
 * its own split-K count (M, N multiples of 256, K >= 512), 2 = the same without the half-phase stagger (A/B measurements only). */
int st5_gemm_set_tn_phased(int mode);
/* 128x128 NT kernel: grids of at most max_blocks blocks (one per CU) use an nbuf-stage operand ring (2 = never; default 256, 4). */
int st5_gemm_set_deep_ring(int max_blocks, int nbuf);
/* 128x128 NT kernel on grids of more than one block per CU: 5 (default) = operand tiles through a ring of five 16 KB LDS slots (A and B
 * of a k-step are separate ring entries: 2.5 k-steps of loads in flight, 80 KB, two blocks per CU), 4 = two whole stages (64 KB).
 * Bit-identical results; A/B switch. */
int st5_gemm_set_nt_slots(int slots);
/* Batch the slab reductions of split-K GEMMs (weight gradients): while enabled, a split-K st5_gemm only queues its reduction;
 * st5_gemm_flush_splitk launches ONE kernel that folds every queued reduction into its output (the outputs are complete
 * only after the flush; same stream as the GEMMs).  Used by the data-parallel wrapper, which flushes before it reduces a
 * gradient bucket across ranks and at the end of backward.  Disabling flushes. */
/* MX-fp8 NT GEMM for the d = 1024 / FFN 4096 Linears of t5_transformer_large (models/speecht5.py:1402-1425; BASELINE.json
 * configs[4]): C = epilogue(A . B^T) with the epilogue features of st5_gemm, A [M x K] and B [N x K] as OCP fp8 e4m3 bytes
 * (p->A / p->B: ld in bytes, K-major, no row split / segments / batch, K % 128 == 0) and one e8m0 scale byte per 32 consecutive
 * k-elements of a row (a_scale [M x K/32], b_scale [N x K/32], row pitches % 4 == 0): element = fp8 * 2^(scale - 127), the OCP
 * microscaling (MX) format consumed directly by v_mfma_scale_f32_32x32x64_f8f6f4.  C-class operands (C, R, P, Cpre) are bf16.
 * Replaces the same F.linear call sites as st5_gemm when the fp8 compute mode is on (speecht5_amd.functional.set_fp8). */
int st5_gemm_mxfp8(const st5_gemm_params* p, const uint8_t* a_scale, int64_t a_scale_ld, const uint8_t* b_scale, int64_t b_scale_ld,
                   void* stream);
/* st5_gemm_mxfp8 whose bf16 output C [M x N] (N % 32 == 0, plain layout) is ALSO written as its MX-fp8 image -- out_q [M x N] e4m3 bytes,
 * out_s [M x N/32] e8m0 scale bytes: the bytes st5_quant_mxfp8 would produce from C -- by the epilogue, for the two producers whose output is
 * the next fp8 GEMM's A operand: bias + GELU with the pre-activation copy (fc1 forward, transformer_layer.py:127-131) and x act'(P) (the data
 * gradient of fc2).  Any other epilogue combination: ST5_ERR_ARG. */
int st5_gemm_mxfp8_q(const st5_gemm_params* p, const uint8_t* a_scale, int64_t a_scale_ld, const uint8_t* b_scale, int64_t b_scale_ld,
                     void* out_q, int64_t out_q_ld, uint8_t* out_s, int64_t out_s_ld, void* stream);
/* Block tile of st5_gemm_mxfp8: 0 (default) = per problem -- the phased 256x256 kernel (gemm_nt8p_mx8_kernel: st5_gemm's phased bf16
 * schedule on fp8 bytes, twice the reduction depth per LDS byte and matrix-pipe cycle) for problems of several rounds of 256x256 tiles
 * or one nearly full round, else 128x128; 1 = 128x128 always, 2 = phased 256x256 always.  Results are bit-identical for every choice. */
int st5_gemm_set_mx8_tile(int mode);
/* The per-problem choice keeps launches with a heavy epilogue (GELU / its derivative, pre-activation copy, dropout, fp8 image) on 128x128
 * tiles, two blocks per CU, unless the reduction has at least `nk` k-tiles of 128 (default 16; 0 = no such rule).  A/B knob. */
int st5_gemm_set_mx8_heavy_nk(int nk);
/* MX quantisation along rows of a bf16 matrix x [rows x cols] (ld elements, cols % 32 == 0): q = e4m3(x * 2^(127 - s)) bytes
 * (pitch q_ld), s[r][c / 32] = floor(log2(max|finite block elements|)) - 8 + 127 as e8m0 (pitch s_ld); round to nearest even, finite
 * values saturating at +-448.  NaN / Inf propagate: the element becomes the e4m3 NaN code 0x7f and its block's scale the e8m0 NaN 0xff,
 * so a diverged tensor still turns the GEMM output (and the loss / gradient norm behind it) non-finite. */
int st5_quant_mxfp8(const void* x, int64_t ld, void* q, int64_t q_ld, uint8_t* s, int64_t s_ld, int64_t rows, int32_t cols, void* stream);
/* The same for njobs CONTIGUOUS bf16 matrices in one launch -- the fp8 images of every eligible Linear weight and of its transposed copy
 * (forward / data-gradient operand of F.linear, transformer_layer.py:127-131,385-389), refreshed once per optimizer step.  jobs: DEVICE array
 * of njobs records { const void* x; void* q; uint8_t* s; int64_t elems (rows * cols, cols % 32 == 0); int32_t cols; int32_t blk0 }, blk0 = the
 * job's first block at 2048 elements per block (ascending, job 0 at 0); nblocks = the total. */
int st5_multi_quant_mxfp8(const void* jobs, int32_t njobs, int32_t nblocks, void* stream);
/* n <= 8 weight-gradient GEMMs (each as st5_gemm would take it: A, B k-strided bf16, ST5_GEMM_OUT_F32, no epilogue but beta and asum; the
 * four / six weight gradients of a transformer layer: autograd of F.linear at transformer_layer.py:127-131,385-389, multihead_attention.py:
 * 213-231,397) as ONE launch in which every block runs the whole token reduction of its tile -- no split-K slabs, no reduction kernel.  The
 * operands must stay valid until the launch has run (the caller queues the problems and keeps the tensors).  A problem's result is
 * independent of what it is grouped with (bit for bit).  A group with a problem of another form, or with two problems writing the same
 * output, runs through st5_gemm one by one. */
int st5_gemm_tn_group(const st5_gemm_params* list, int32_t n, int dtype, void* stream);
/* Block tile of st5_gemm_tn_group: 0 (default) = per problem -- the phased 256x256 grouped kernel (gemm_tn8p_group_kernel: whole token
 * reductions on st5_gemm's phased schedule; weight gradients bit-identical to the 128x128 group, bias-gradient column summed on the VALU in
 * its own fixed order) when M and N are multiples of 256 and K >= 512, i.e. every Linear of the transformer; 1 = 128x128 always. */
int st5_gemm_set_tn_group_tile(int mode);
/* 1 when st5_gemm_tn_group would run a weight gradient of this shape on the phased kernel (host-side accounting of 256x256 tiles). */
int st5_gemm_tn_group_is_phased(int32_t M, int32_t N, int32_t K);
int st5_gemm_defer_splitk(int enabled, void* stream);
int st5_gemm_flush_splitk(void* stream);

/* ---- row-wise normalisation (encoder.py:226, transformer_layer.py:124,132, speech_encoder_prenet.py:174) */
/* y = LN(x) * gamma + beta over the last dim (cols); saves mean/rstd (fp32 [rows]). */
int st5_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean,
                      float* rstd, int64_t rows, int32_t cols, float eps, int dtype, void* stream);
/* dx; dgamma/dbeta are ACCUMULATED (+=) into fp32 [cols]; ws >= st5_layernorm_bwd_ws_bytes(). */
int st5_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                      float* dgamma, float* dbeta, void* ws, int64_t rows, int32_t cols,
                      void* dx_dropped /* optional 2nd output dx * dropout_mask(seed, row*cols + c): the gradient of the
                                          dropout-epilogue Linear in front of this LayerNorm (cols % 4 == 0) */,
                      float drop_p, uint64_t drop_seed, int dtype, void* stream);
/* Batched dgamma / dbeta reductions: while enabled, st5_layernorm_bwd leaves its block partials in an internal arena and
 * st5_layernorm_flush(stream) folds all pending LayerNorms' partials into their dgamma / dbeta with ONE launch (same stream
 * as the st5_layernorm_bwd calls; the owner of the gradient buffers flushes wherever gradients must be complete). */
/* st5_layernorm_fwd for bf16 rows with cols % 32 == 0 (cols <= 2048) that also writes y's MX-fp8 image (q [rows x cols] e4m3 bytes,
 * sc [rows x cols / 32] e8m0 scale bytes: the bytes st5_quant_mxfp8 produces from y): the LayerNorm in front of the QKV projection / fc1 of
 * a pre-LN layer in fp8 compute mode (transformer_layer.py:103-110,124-126 with `encoder_normalize_before`). */
int st5_layernorm_fwd_q8(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, void* q, uint8_t* sc,
                         int64_t rows, int32_t cols, float eps, void* stream);
/* st5_layernorm_bwd whose dx also receives `addend` (dx = LayerNorm backward + addend; same shape / dtype as dx, cols % 4 == 0, cols <= 2048):
 * the gradient of a pre-LN block's residual connection (transformer_layer.py:90-111 with layer_norm_first: y = x + f(LN(x))) folded into
 * the LayerNorm backward at the block's input instead of an autograd accumulation kernel. */
int st5_layernorm_bwd_add(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                          float* dbeta, void* ws, int64_t rows, int32_t cols, const void* addend, int dtype, void* stream);
/* y = GELU(LN(x) * gamma + beta) in ONE pass and its backward (dx, dgamma += , dbeta += from the gradient of the activated output; LN(x) is
 * recomputed, nothing but x, mean, rstd is kept): the LayerNorm + GELU behind every convolution of the layer-norm feature extractor
 * (t5_transformer_large: speech_encoder_prenet.py:318-331 with extractor_mode=layer_norm).  cols % 4 == 0, cols <= 512; bf16 uses the GELU
 * polynomials of the GEMM epilogues, fp32 the exact erf form.  ws as st5_layernorm_bwd_ws_bytes(rows, cols). */
int st5_layernorm_gelu_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int64_t rows, int32_t cols,
                           float eps, int dtype, void* stream);
int st5_layernorm_gelu_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd, void* dx,
                           float* dgamma, float* dbeta, void* ws, int64_t rows, int32_t cols, int dtype, void* stream);
/* The LayerDrop gate folded into a post-LN layer's LAST LayerNorm (modules/encoder.py:251-257, modules/decoder.py:64-67 inside a
 * replayed step, see st5_select): forward  y = *keep ? LN(x) * gamma + beta : skip  (skip = the layer's input, same shape and dtype);
 * backward  as st5_layernorm_bwd with dy counted as zero when *keep == 0 (dx = 0, nothing added to dgamma / dbeta).  The gradient
 * of the layer's OUTPUT then reaches the layer's input through st5_skip_grad.  keep = one float in device memory; cols % 4 == 0. */
int st5_layernorm_gated_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int64_t rows,
                            int32_t cols, float eps, const float* keep, const void* skip, int dtype, void* stream);
int st5_layernorm_gated_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                            float* dgamma, float* dbeta, void* ws, int64_t rows, int32_t cols, void* dx_dropped, float drop_p,
                            uint64_t drop_seed, const float* keep, int dtype, void* stream);
/* The LayerDrop LAYER GATE (st5_gemm_params.gate): inside a replayed step a dropped layer cannot be skipped on the host, so every launch
 * of a gated layer carries the layer's keep float and exits at once when *gate == 0.  Rule for what a dropped launch leaves behind: DEAD
 * outputs (read only by launches of the same layer) are not written at all; LIVE outputs (read outside the layer) get what a dropped layer
 * gives today -- exact zeros, or an unchanged accumulator.  gate NULL or *gate != 0: the ungated call, bit for bit.
 * st5_layernorm_fwd_gate: st5_layernorm_fwd (keep == skip == NULL) or st5_layernorm_gated_fwd (both given; pass the same pointer as gate).
 * Dropped: a plain LayerNorm writes nothing; the gated one writes y = skip without reading x; mean / rstd stay unwritten.
 * st5_layernorm_bwd_gate: st5_layernorm_bwd (keep NULL) or st5_layernorm_gated_bwd.  Dropped: dy, x, mean, rstd are not read, dx / dx_dropped
 * not written, nothing is added to dgamma / dbeta (zero block partials: also through st5_layernorm_defer / _flush).
 * Vector kernels only (cols % 4 == 0, cols <= 2048, dx given): anything else with a gate is ST5_ERR_ARG, never an ungated fall-back. */
int st5_layernorm_fwd_gate(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int64_t rows,
                           int32_t cols, float eps, const float* keep, const void* skip, const float* gate, int dtype, void* stream);
int st5_layernorm_bwd_gate(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                           float* dbeta, void* ws, int64_t rows, int32_t cols, void* dx_dropped, float drop_p, uint64_t drop_seed,
                           const float* keep, const float* gate, int dtype, void* stream);
int st5_layernorm_defer(int enabled, void* stream);
int st5_layernorm_flush(void* stream);
int64_t st5_layernorm_bwd_ws_bytes(int64_t rows, int32_t cols);

/* ---- attention probabilities (multihead_attention.py:343-386) ----
 * scores [BH, T, lds] (dtype) hold alpha*q.k^T; qp [BH, T, nb] (dtype) holds alpha*q.pe^T (may be NULL);
 * P[bh,i,j] = softmax_j(scores + qp[bh,i,clip(i-j,-maxrel,maxrel-1)+maxrel] + causal + key-padding(-inf)).
 * Writes probs (dtype, [BH,T,lds], pad cols zeroed) and, when dropout_p > 0, probs_drop (dropout applied).
 * kpm: uint8 [B, S] (1 = padded key) or NULL.  H = heads (bh = b*H + h). */
int st5_softmax_fwd(const void* scores, const void* qp, const uint8_t* kpm, void* probs, void* probs_drop,
                    int32_t BH, int32_t H, int32_t T, int32_t S, int32_t lds, int32_t nb, int32_t maxrel,
                    int32_t causal, float dropout_p, uint64_t seed, int dtype, void* stream);
/* dS = P * (dP' - sum_j dP'_j P_j), dP' = dropout'(dP) (+ dP_extra fp32 on the un-dropped probs);
 * dqp[bh,i,b] (dtype, fully written by the kernel) = sum_{j: bucket(i-j)=b} dS[bh,i,j]. dS overwrites dP. */
int st5_softmax_bwd(void* dP_inout, const void* probs, const float* dP_extra, void* dqp, int32_t BH, int32_t T,
                    int32_t S, int32_t lds, int32_t nb, int32_t maxrel, float dropout_p, uint64_t seed, int dtype,
                    void* stream);

/* ---- fused attention (bf16, head_dim 64): O = dropout(softmax(scale*Q.K^T + relpos-bias + masks)) . V without
 *      materialising scores (multihead_attention.py:340-389).  q/k/v/o are row-major projections with leading dimensions
 *      *_ld: row (b*T + t) (queries) / (b*S + s) (keys), column h*64 + d.  lse fp32 [B*H, T] (saved for backward).
 *      pe: relative key table [nb = 2*maxrel, 64] (dtype) or NULL.  lds: row length used by the dropout counter
 *      (same generator/counters as the unfused st5_softmax path).  Other dtypes / head sizes: use the unfused path. */
int st5_flash_attn_fwd(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld, void* o,
                       int64_t o_ld, float* lse, const void* pe, const uint8_t* kpm, int32_t B, int32_t H, int32_t T,
                       int32_t S, int32_t head_dim, int32_t nb, int32_t maxrel, int32_t causal, int32_t lds, float scale,
                       float dropout_p, uint64_t seed, int dtype, void* stream);

/* Relative-position table of the fused kernels: QP[bh][q][row] (dtype) with row = st5_flash_attn_qp_row(nb) elements:
 * second-generation kernels (default): [8 x QP[0] | scale*log2(e) * q.pe[b]^T, b = 0..nb-1 | 8 x QP[nb-1]] -- the replicated
 * end chunks are what a clipped relative position reads, so clipping is a clamp of a 16-byte chunk index; first generation
 * (st5_flash_attn_set_impl(1)): the plain nb values.  The kernels DMA per-tile windows of it into LDS.
 * st5_flash_attn_qp_table builds it (the forward does this itself when given qp_out); the backward takes it as `qp`. */
int32_t st5_flash_attn_qp_row(int32_t nb);
int st5_flash_attn_qp_table(const void* q, int64_t q_ld, const void* pe, void* qp_out, int32_t B, int32_t H, int32_t T, int32_t nb,
                            float scale, int dtype, void* stream);
/* 2 (default): second-generation kernels (csrc/flash_attn2.hip: LDS-DMA staging, transpose reads, bias windows, two blocks per
 * CU); 1: first generation (csrc/flash_attn.hip).  Same results bit for bit; A/B measurements and tests only. */
int st5_flash_attn_set_impl(int impl);

/* st5_flash_attn_fwd with the relative-position table workspace (qp_out [B*H, T, st5_flash_attn_qp_row(nb)], dtype; required by
 * the second-generation kernels when pe != NULL -- without it the call runs the first-generation kernel, which keeps the table
 * in LDS): built here, returned for the backward's `qp` input. */
int st5_flash_attn_fwd_qp(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld, void* o,
                          int64_t o_ld, float* lse, const void* pe, const uint8_t* kpm, int32_t B, int32_t H, int32_t T,
                          int32_t S, int32_t head_dim, int32_t nb, int32_t maxrel, int32_t causal, int32_t lds, float scale,
                          float dropout_p, uint64_t seed, void* qp_out, int dtype, void* stream);

/* st5_flash_attn_fwd_qp with the layer gate: *gate == 0 -> the table kernel and the attention kernel exit; o, lse, qp_out are not written.
 * Second-generation kernels only (a gate with st5_flash_attn_set_impl(1), or with pe but no qp_out, is ST5_ERR_ARG). */
int st5_flash_attn_fwd_qp_gate(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld, void* o,
                               int64_t o_ld, float* lse, const void* pe, const uint8_t* kpm, int32_t B, int32_t H, int32_t T,
                               int32_t S, int32_t head_dim, int32_t nb, int32_t maxrel, int32_t causal, int32_t lds, float scale,
                               float dropout_p, uint64_t seed, void* qp_out, const float* gate, int dtype, void* stream);

/* Backward of st5_flash_attn_fwd: recomputes P from (q, k, bias, lse).  Writes dq/dk/dv (dtype, same row layouts as
 * q/k/v with their own leading dimensions); dvec fp32 [B*H*T] scratch (D = rowsum(dO*O)).  With pe: qp = the relative-position table
 * [B*H, T, st5_flash_attn_qp_row(nb)] (from st5_flash_attn_fwd_qp or st5_flash_attn_qp_table) and dqp [B*H, T, nb] (plain) receives the bucket gradients
 * (the caller folds dqp into dq and d(pe) with st5_gemm, exactly as for the unfused path). */
int st5_flash_attn_bwd(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld, const void* o,
                       int64_t o_ld, const void* dout, int64_t do_ld, void* dq, int64_t dq_ld, void* dk, int64_t dk_ld, void* dv,
                       int64_t dv_ld, const float* lse, float* dvec, const void* pe, const void* qp, void* dqp,
                       const uint8_t* kpm, int32_t B, int32_t H, int32_t T, int32_t S, int32_t head_dim, int32_t nb,
                       int32_t maxrel, int32_t causal, int32_t lds, float scale, float dropout_p, uint64_t seed, int dtype,
                       void* stream);
/* The same with the dq and dkv kernels side by side: D on `stream`, then dq on `stream` and dkv on `stream2`
 * (ordered after everything enqueued on `stream`), `stream` joined with `stream2` before returning.  stream2 NULL =
 * st5_flash_attn_bwd.  Results are bit-identical to the single-stream form. */
int st5_flash_attn_bwd_2s(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld, const void* o,
                          int64_t o_ld, const void* dout, int64_t do_ld, void* dq, int64_t dq_ld, void* dk, int64_t dk_ld,
                          void* dv, int64_t dv_ld, const float* lse, float* dvec, const void* pe, const void* qp, void* dqp,
                          const uint8_t* kpm, int32_t B, int32_t H, int32_t T, int32_t S, int32_t head_dim, int32_t nb,
                          int32_t maxrel, int32_t causal, int32_t lds, float scale, float dropout_p, uint64_t seed, int dtype,
                          void* stream, void* stream2);

/* st5_flash_attn_bwd_2s with the layer gate: *gate == 0 -> every kernel exits; dq, dqp, dvec are not written.  dkv_live == 0: neither are
 * dk / dv (self-attention: only the layer's own QKV backward reads them).  dkv_live != 0: dk / dv receive exact zeros in the rows and
 * columns the kept kernel writes and nowhere else -- the decoder's cross-attention writes its column slice of the K|V gradient buffer all
 * layers share, which is not zero-filled. */
int st5_flash_attn_bwd_2s_gate(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld, const void* o,
                               int64_t o_ld, const void* dout, int64_t do_ld, void* dq, int64_t dq_ld, void* dk, int64_t dk_ld,
                               void* dv, int64_t dv_ld, const float* lse, float* dvec, const void* pe, const void* qp, void* dqp,
                               const uint8_t* kpm, int32_t B, int32_t H, int32_t T, int32_t S, int32_t head_dim, int32_t nb,
                               int32_t maxrel, int32_t causal, int32_t lds, float scale, float dropout_p, uint64_t seed,
                               const float* gate, int32_t dkv_live, int dtype, void* stream, void* stream2);

/* ---- speech pre-net layer 0: Conv1d(1->C,k,stride,no bias) + GroupNorm(C groups) + GELU
 *      (speech_encoder_prenet.py:300,323-324).  wav fp32 [B,S]; out channels-last [B,L,C] (dtype);
 *      stats fp32 [B,C,2] = (mean, rstd) saved for backward.  ws >= st5_conv0_ws_bytes. */
int st5_conv0_gn_gelu_fwd(const float* wav, const float* w, const float* gamma, const float* beta, void* out,
                          float* stats, void* ws, int32_t B, int32_t S, int32_t C, int32_t k, int32_t stride,
                          float eps, int dtype, void* stream);
/* dY channels-last (dtype).  Accumulates (+=) dw [C,k], dgamma [C], dbeta [C] (fp32), scaled by gscale. */
int st5_conv0_gn_gelu_bwd(const float* wav, const float* w, const float* gamma, const float* beta,
                          const float* stats, const void* dY, float* dw, float* dgamma, float* dbeta, void* ws,
                          int32_t B, int32_t S, int32_t C, int32_t k, int32_t stride, float gscale, int dtype,
                          void* stream);
/* The same pair with the waveform moments carried from the forward to the backward: `mom` = B x st5_conv0_mom_count(k) doubles (sum_t
 * x[s t + j] and sum_t x[s t + j] x[s t + j'], j <= j' < k: what the GroupNorm backward needs of the waveform besides dY).  The forward
 * publishes them (NULL: not), the backward given them skips its own pass over the waveform and the fold (two launches of ~17 us for 4 KB
 * of results); NULL in the backward = st5_conv0_gn_gelu_bwd.  Same results bit for bit: the same kernels produce the same doubles. */
int32_t st5_conv0_mom_count(int32_t k);
int st5_conv0_gn_gelu_fwd_m(const float* wav, const float* w, const float* gamma, const float* beta, void* out, float* stats, double* mom,
                            void* ws, int32_t B, int32_t S, int32_t C, int32_t k, int32_t stride, float eps, int dtype, void* stream);
int st5_conv0_gn_gelu_bwd_m(const float* wav, const float* w, const float* gamma, const float* beta, const float* stats, const double* mom,
                            const void* dY, float* dw, float* dgamma, float* dbeta, void* ws, int32_t B, int32_t S, int32_t C, int32_t k,
                            int32_t stride, float gscale, int dtype, void* stream);
/* The forward with PER-ROW LENGTHS (inference: no moments published, no backward).  `lens` int32 [B] on the device, in samples, of a
 * right-padded batch wav [B,S].  Row b's GroupNorm statistics are taken over its own L_b = (lens[b] - k) / stride + 1 frames; output
 * frames t >= L_b are stored as zeros.  `stats` [b] and the output frames t < L_b are the bits st5_conv0_gn_gelu_fwd gives for the
 * single-row call on wav[b, :lens[b]], in every fold / mfma setting (the fold groups the chunk partials by chunk parity and adds each
 * group in index order, whatever the launch-wide chunk count; the chunks past a row's end contribute + 0.0).  Lengths outside
 * [k, S] are clamped into the launch's frame range (a row shorter than k gets L_b = 0: all-zero output, undefined statistics); the
 * caller validates them. */
int st5_conv0_gn_gelu_fwd_rows(const float* wav, const int32_t* lens, const float* w, const float* gamma, const float* beta, void* out,
                               float* stats, void* ws, int32_t B, int32_t S, int32_t C, int32_t k, int32_t stride, float eps, int dtype,
                               void* stream);
/* A/B switch of the bf16 forward apply pass: 1 (default) = convolution on the matrix cores with split-bf16 operands (x = xh + xl,
 * w = wh + wl; wh.xh + wh.xl + wl.xh in two v_mfma_f32_32x32x16_bf16 per 32 channels x 32 steps), 0 = the VALU form. */
int st5_conv0_set_mfma(int on);
/* A/B switch of the matrix-core forward: 1 (default) = the clip's GroupNorm statistics and the weight fragments come from one launch
 * (moments, statistics + fragments, apply: three launches), 0 = separate statistics and fragment launches (four).  `stats` holds the
 * same bits either way. */
int st5_conv0_set_fold(int on);
/* A/B switch of the matrix-core forward's GELU: 1 (default) = a 256-entry chord table of the upper tail Q = 1 - Phi in LDS,
 * gelu(z) = max(z, 0) - |z| Q(|z|) (|error| <= 8.4e-6 |z|, 8.5 VALU issue slots per element), 0 = the transcendental-free
 * polynomial (1.5e-5 |z|, 14.5 slots). */
int st5_conv0_set_gelu_table(int on);
int64_t st5_conv0_ws_bytes(int32_t B, int32_t S, int32_t C, int32_t k, int32_t stride);

/* ---- element-wise / reductions (glue ops fused where the reference has separate torch calls) */
/* Alignment rule of the FLAT entry points (st5_cast_from_f32 without transpose, st5_cast_to_f32, st5_sumsq, st5_sumsq_pair, st5_axpby,
 * st5_act_fwd, st5_act_bwd, st5_dropout): pointers need only the alignment of their element type.  16-byte vectors when every pointer
 * argument is 16-byte aligned, scalars otherwise -- the same arithmetic per element, so every element comes out with the same bits
 * either way (the two sums: see st5_sumsq). */
/* dst(dtype) = src(fp32), optionally transposed: src [rows, cols] -> dst [cols, rows].  Round to nearest even.  Not transposed: 16-byte
 * vectors when src and dst are 16-byte aligned, scalars otherwise (same bits). */
int st5_cast_from_f32(const float* src, void* dst, int64_t rows, int64_t cols, int32_t transpose, int dtype,
                      void* stream);
/* dst(fp32) = src(dtype).  16-byte vectors when src and dst are 16-byte aligned, scalars otherwise (same bits). */
int st5_cast_to_f32(const void* src, float* dst, int64_t n, int dtype, void* stream);
/* out[c] (+)= scale * sum_r x[r, c]   (bias gradients); ws >= st5_colsum_ws_bytes(rows, cols) */
int st5_colsum_ws(const void* x, float* out, void* ws, int64_t rows, int32_t cols, int64_t ld, float scale,
                  int32_t accumulate, int dtype, void* stream);
/* st5_colsum_ws with the layer gate (see st5_layernorm_fwd_gate): *gate == 0 -> x and the partials are not read; the overwrite form stores
 * exact zeros (a dropped layer's relative-position gradient, read outside the layer), the accumulating form leaves `out` alone. */
int st5_colsum_ws_gate(const void* x, float* out, void* ws, int64_t rows, int32_t cols, int64_t ld, float scale, int32_t accumulate,
                       const float* gate, int dtype, void* stream);
int64_t st5_colsum_ws_bytes(int64_t rows, int32_t cols);
/* Relative-position part of the self-attention backward in one launch (bf16, head_dim 64; csrc/relpos_bwd.hip).  dqp [B*H, T, nb] are the
 * bucket gradients the dkv kernel wrote; q / dq point at head 0 of batch 0 of a [B*T, ld] buffer (head h at column 64 h); pe [nb, 64].
 *   dq[bh][t][:]    = bf16(alpha * (dqp[bh][t][:] . pe) + dq[bh][t][:])      (read and written)
 *   part[bh][b][:]  = alpha * sum_t dqp[bh][t][b] * q[bh][t][:]              (fp32 [B*H, nb, 64]; part == NULL: the dq half alone)
 * Both are the bytes st5_gemm produces for the same operands (NT with beta = 1; k-strided A and B with ST5_GEMM_OUT_F32).  Rows t >= T
 * are neither read into the sums nor written.  nb: see st5_relpos_bwd_supported.  gate (may be NULL): the layer gate, *gate == 0 ->
 * nothing is read, dq and part are left unwritten. */
int st5_relpos_bwd(const void* dqp, const void* q, int64_t q_ld, const void* pe, void* dq, int64_t dq_ld, float* part, int32_t B, int32_t H,
                   int32_t T, int32_t nb, float alpha, const float* gate, int dtype, void* stream);
int st5_relpos_bwd_supported(int32_t nb);   /* nb a multiple of 64, at most 320 (the partial lives in accumulator registers) */
/* dpe[c] (dtype) = sum over rows of part[r][c], in the order of st5_colsum_ws (overwrite form, scale 1) followed by st5_cast_from_f32: same
 * bytes, one launch.  gate (may be NULL): *gate == 0 -> part is not read, dpe = exact zeros. */
int st5_relpos_dpe_final(const float* part, void* dpe, int64_t rows, int32_t cols, const float* gate, int dtype, void* stream);
/* out[0] (+)= scale * sum(x^2)   (features_pen, speech_encoder_prenet.py:172).  16-byte vectors when x is 16-byte aligned, scalars
 * otherwise: the squares are then added in ANOTHER ORDER (one element per thread and trip instead of eight), so the sum over an unaligned
 * buffer may differ in its last bits from the sum of the same values at an aligned address.  st5_sumsq (fp32) and st5_sumsq_pair walk
 * the same partition on the same alignment (for the pair: x and y both aligned / not both aligned) and agree bit for bit there. */
int st5_sumsq(const void* x, float* out, int64_t n, float scale, int32_t accumulate, int dtype, void* stream);
/* y = a*x + b*y in place.  16-byte vectors when x and y are 16-byte aligned, scalars otherwise (same bits). */
int st5_axpby(const void* x, void* y, int64_t n, float a, float b, int dtype, void* stream);
/* LayerDrop inside a replayed (HIP-graph) step, where the host's per-layer draw cannot steer control flow
 * (modules/encoder.py:251-257 `if not self.training or (dropout_probability > self.encoder_layerdrop)`, modules/decoder.py:64-67
 * LayerDropModuleList): every layer runs and  y = keep ? b (layer output) : a (layer input),  keep = one float in device memory
 * written from the host draw before the replay; backward (ga, gb) = keep ? (0, g) : (g, 0).  Raw 16-byte chunks, any dtype. */
int st5_select(const float* keep_dev, const void* a, const void* b, void* y, int64_t nbytes, void* stream);
int st5_select_bwd(const float* keep_dev, const void* g, void* ga, void* gb, int64_t nbytes, void* stream);
/* dx = *keep ? dx : g  in place (raw 16-byte chunks): the input gradient of a gated layer (st5_layernorm_gated_fwd) -- a kept layer's
 * own input gradient stands, a dropped layer's (exact zeros) is replaced by the gradient of its output. */
int st5_skip_grad(const float* keep_dev, const void* g, void* dx, int64_t nbytes, void* stream);
/* y = act(x) ; dx = dy * act'(x).  y may be x, dx may be dy.  A NaN in x comes out of every activation's forward as NaN (ReLU
 * included, as torch.relu gives it).  16-byte vectors when every pointer is 16-byte aligned, scalars otherwise (same bits). */
int st5_act_fwd(const void* x, void* y, int64_t n, int32_t act, int dtype, void* stream);
int st5_act_bwd(const void* dy, const void* x, void* dx, int64_t n, int32_t act, int dtype, void* stream);
/* y[r,c] = act(x[r,c] * a[c] + b[c])   (per-channel affine: spectrogram normalisation, BatchNorm apply) */
int st5_channel_affine(const void* x, const float* a, const float* b, void* y, int64_t rows, int32_t cols, int32_t act,
                       int dtype, void* stream);
/* y = dropout(x) with the library's counter RNG (same generator as the GEMM epilogue), counter = the element's index.  16-byte vectors
 * when x and y are 16-byte aligned, scalars otherwise (same mask, same bits). */
int st5_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, int dtype, void* stream);
/* x[r,:] = v (fp32 [cols]) where mask[r] != 0  (apply_hubert_mask, speech_encoder_prenet.py:249) */
int st5_masked_fill_rows(void* x, const uint8_t* mask, const float* v, int64_t rows, int32_t cols, int dtype,
                         void* stream);
/* dv[c] += sum_{r: mask[r]} dx[r,c]; dx[r,:] = 0 where mask[r] */
int st5_masked_fill_rows_bwd(void* dx, const uint8_t* mask, float* dv, int64_t rows, int32_t cols, int dtype,
                             void* stream);
/* y[r,:] = x[r,:] + scale * table[idx[r], :]   (table fp32 [n, cols]); idx int32 [rows] */
int st5_add_table_rows(const void* x, const float* table, const int32_t* idx, void* y, int64_t rows, int32_t cols,
                       float scale, int dtype, void* stream);
/* same with the scale read from device memory (learnable alpha of ScaledPositionalEncoding; no host sync) */
int st5_add_table_rows_dev(const void* x, const float* table, const int32_t* idx, void* y, int64_t rows, int32_t cols,
                           const float* scale_dev, int dtype, void* stream);
/* y[r,:] = emb_scale * table[tok[r],:] + pos_scale * pos[pidx[r],:]   (embedding + positions) */
int st5_embed_rows(const float* table, const int32_t* tok, const float* pos, const int32_t* pidx, void* y,
                   int64_t rows, int32_t cols, float emb_scale, float pos_scale, int dtype, void* stream);
/* dtable[tok[r],:] += scale * dy[r,:]  (fp32 atomics) */
int st5_embed_rows_bwd(const void* dy, const int32_t* tok, float* dtable, int64_t rows, int32_t cols, float scale,
                       int dtype, void* stream);
/* The same, bit-reproducible (no atomics): the rows are rank-sorted by (table row, position) and every table row is summed in
 * position order by one block.  Tokens outside [0, vocab) contribute nothing; cols % 4 == 0.  The sort is quadratic in `rows` (one micro-batch
 * of tokens / frames: ~10 us for 8k rows); rows <= 2^22.  Uses one internal workspace: calls must be stream-ordered. */
int st5_embed_rows_bwd_det(const void* dy, const int32_t* tok, float* dtable, int64_t rows, int32_t cols, int32_t vocab, float scale,
                           int dtype, void* stream);
/* ... with a per-row weight: row r is scaled by row_w[(r / rw_div) % rw_mod] (NULL = 1). */
int st5_embed_rows_bwd_det_w(const void* dy, const int32_t* tok, float* dtable, int64_t rows, int32_t cols, int32_t vocab, float scale,
                             const float* row_w, int32_t rw_div, int32_t rw_mod, int dtype, void* stream);
/* dst[a, b, c] (+)= src[off + a*sa + b*sb + c*sc]  (src fp32, dst `dtype`, element strides, may be negative): one-pass weight
 * re-layout + cast for the implicit-GEMM convolutions, and re-laid-out accumulation of their weight gradients. */
int st5_gather3(const float* src, void* dst, int32_t A, int32_t B, int32_t C, int64_t sa, int64_t sb, int64_t sc, int64_t off,
                int32_t accumulate, int dtype, void* stream);
/* x[b, t, :] = 0 for t < head and for t >= tail_start (x [B, Tp, C]): halo rows + rows no output window covers, one launch. */
int st5_zero_time_edges(void* x, int32_t B, int32_t Tp, int32_t C, int32_t head, int32_t tail_start, int dtype, void* stream);
/* zero-padded copy: dst [B, pad_l + T + pad_r, C] <- src [B, T, C] */
/* out[(b,t), j] = wav[b, t*stride + j] (j < k), 0 (k <= j < kpad); out is [B*L, kpad] (dtype), L = (S-k)/stride + 1.
 * Turns the Cin = 1 first convolution of the extractor_mode=layer_norm feature extractor
 * (speech_encoder_prenet.py:300-318) into rows for st5_gemm. */
int st5_unfold_rows(const float* wav, void* out, int32_t B, int32_t S, int32_t k, int32_t stride, int32_t kpad, int dtype,
                    void* stream);
int st5_pad_time(const void* src, void* dst, int32_t B, int32_t T, int32_t C, int32_t pad_l, int32_t pad_r,
                 int dtype, void* stream);
/* HiFi-GAN generator (HuggingFace SpeechT5HifiGan, modeling_speecht5.py:2887-3066: every convolution is preceded by a LeakyReLU
 * and zero "same" padding): dst [B, pad_l + T + pad_r, C] = zero-padded act(src [B, T, C]) in ONE pass (16-byte vectors when
 * C * sizeof(elem) % 16 == 0), act in {ST5_ACT_NONE, ST5_ACT_LRELU_01, ST5_ACT_LRELU_001, ...} with act(0) == 0. */
int st5_pad_time_act(const void* src, void* dst, int32_t B, int32_t T, int32_t C, int32_t pad_l, int32_t pad_r, int32_t act,
                     int dtype, void* stream);
/* Zero the halo rows [0, pad_l) and [pad_l + T, pad_l + T + pad_r) of every batch element of dst [B, pad_l + T + pad_r, C]: a
 * convolution whose st5_gemm output operand addresses the interior of the padded buffer the NEXT convolution reads. */
int st5_zero_halo(void* dst, int32_t B, int32_t T, int32_t C, int32_t pad_l, int32_t pad_r, int dtype, void* stream);
/* ---- ragged (packed) batches of the text-to-waveform path (csrc/ragged.hip; speecht5_amd/ragged.py builds the tables once per
 *      call): B utterances lie one after another along time, each followed by a gap of G mel frames; at a stage of cumulative
 *      upsampling rate s mel frame f covers rows [s*f, s*(f+1)).  valid: one byte per mel frame (1 inside an utterance, 0 in a gap).
 *      st5_ragged_pad_act: st5_pad_time_act for one packed sequence, dst [pad_l + frames*s + pad_r, C] row t' =
 *      act(src[t' - pad_l]) where valid[(t' - pad_l) / s], else 0 -- a select, so whatever lies in a gap row of src never reaches
 *      dst.  st5_ragged_zero_gaps: rows [s*f, s*(f+1)) of buf [frames*s, C] := 0 for the n_gap frames listed in gap_frames (work
 *      proportional to the gaps; a listed frame that is out of range or marked valid is skipped, so a valid row is never written):
 *      for buffers a convolution's or the BatchNorm kernel's epilogue wrote.  st5_ragged_gather_rows: dst[u, 0:w] =
 *      src[idx[u], 0:w], or 0 when idx[u] is outside [0, src_rows); fp32 -> `dtype` (to_f32 = 0: packing fp32 records, gap rows
 *      zero) or `dtype` -> fp32 (to_f32 = 1: unpacking the packed waveform / mel into per-row results). */
int st5_ragged_pad_act(const void* src, void* dst, const uint8_t* valid, int64_t frames, int32_t s, int32_t C, int32_t pad_l,
                       int32_t pad_r, int32_t act, int dtype, void* stream);
int st5_ragged_zero_gaps(void* buf, const uint8_t* valid, const int32_t* gap_frames, int64_t n_gap, int64_t frames, int32_t s,
                         int32_t C, int dtype, void* stream);
int st5_ragged_gather_rows(const void* src, const int32_t* idx, void* dst, int64_t n_rows, int64_t src_rows, int32_t w,
                           int32_t to_f32, int dtype, void* stream);
/* Channels-last Conv1d with 32 or 64 OUTPUT channels, bf16, as an MFMA implicit GEMM whose 32 MFMA rows are the output channels and
 * whose columns are time steps (csrc/conv1d_narrow.hip) -- the 64- and 32-channel stages of the HiFi-GAN generator (HF
 * modeling_speecht5.py:2920-2960 residual blocks, :3010-3030 upsampler), where the 128-wide tiles of st5_gemm waste 1/2 .. 3/4 of
 * their MFMAs:
 *   y[b, t, co] = act(alpha * sum_{tau < taps, c < Cin} w[co, tau * Cin + c] * x[b, t, tau, c] + bias[co]) + residual[b, t, co] + beta * y[b, t, co]
 * with x[b, t, tau, c] = x[b * x_bs + t * x_ts + tau * tap_stride + c] (all strides in ELEMENTS; the caller's buffer holds the halo rows:
 * a dilated convolution is tap_stride = dilation * Cin over the zero-padded input, one phase of a stride-s transposed convolution is
 * taps = 2, tap_stride = Cin), y / residual addressed as base + b * bs + t * ts + co (padded or phase-interleaved layouts without
 * copies).  Cin in {32, 64, 128}, Cout in {32, 64}; x, w 16-byte aligned, y and residual 8-byte aligned, strides multiples of
 * 8 (x) / 4 (y, residual) elements, else ST5_ERR_ARG / ST5_ERR_ALIGN.  The weight image lives in LDS:
 * Cout * (taps * Cin + 8) * 2 bytes <= 160 KB, else ST5_ERR_ARG (nothing is launched).  act in {ST5_ACT_NONE, ST5_ACT_LRELU_01,
 * ST5_ACT_LRELU_001}, else ST5_ERR_ARG.  bias fp32 or NULL; residual NULL for none. */
int st5_conv1d_narrow(const void* x, int64_t x_bs, int32_t x_ts, const void* w, const float* bias, void* y, int64_t y_bs, int32_t y_ts,
                      const void* residual, int64_t r_bs, int32_t r_ts, int32_t B, int32_t L, int32_t Cin, int32_t Cout, int32_t taps,
                      int32_t tap_stride, float alpha, float beta, int32_t act, void* stream);
/* What st5_conv1d_narrow would run for these arguments, host only (nothing is launched or dereferenced): the error code the launch would
 * return, and on ST5_OK plan[0..5] = { staged (1: the LDS-staged 32-channel form conv1d_narrow32_kernel<NJ>, 0: the direct form
 * conv1d_narrow_kernel<CB, NJ>), CB = Cout / 32, NJ = Cin / 16, tiles per block, time steps per block tile (1024; 512 for Cout = 64),
 * dynamic LDS bytes }.  The staged form needs Cout = 32, Cin in {32, 64}, x_ts == Cin, tap_stride % Cin == 0, y / residual 16-byte
 * aligned with strides multiples of 8, and its LDS image (weights + 8 waves x (128 + (taps - 1) tap_stride / Cin) rows of 2 Cin + 16
 * bytes) within 160 KB; ST5_NARROW_V1=1 in the environment selects the direct form throughout.  st5_conv1d_narrow takes its dispatch
 * from the same function. */
int st5_conv1d_narrow_plan(const void* x, int64_t x_bs, int32_t x_ts, const void* w, const float* bias, void* y, int64_t y_bs, int32_t y_ts,
                           const void* residual, int64_t r_bs, int32_t r_ts, int32_t B, int32_t L, int32_t Cin, int32_t Cout, int32_t taps,
                           int32_t tap_stride, float alpha, float beta, int32_t act, int32_t* plan);
/* The generator's last convolution (HF modeling_speecht5.py:3058-3062: 32 -> 1 channels, k = 7, tanh), bf16:
 *   y[b * L + t] = act(alpha * sum_{tau, c} w[tau * Cin + c] * x[b * x_bs + t * x_ts + tau * tap_stride + c] + bias[0]). */
int st5_conv1d_cout1(const void* x, int64_t x_bs, int32_t x_ts, const void* w, const float* bias, void* y, int32_t B, int32_t L, int32_t Cin,
                     int32_t taps, int32_t tap_stride, float alpha, int32_t act, void* stream);

/* ---- log-mel front end of the input pipeline (data/speech_dataset.py:142-181 `logmelfilterbank`: librosa.stft
 *      n_fft 1024 / hop 256 / periodic Hann / centred with reflect padding, |.|, 80 Slaney mel filters, log10 floor 1e-10).
 *      The two matrix products (windowed DFT basis, mel filterbank) are st5_gemm calls in fp32; these are the pieces around them.
 *      st5_stft_frames: out fp32 [B * L, n_fft], L = 1 + S / hop, out[(b,l), j] = wav[b, reflect(l*hop + j - n_fft/2)].
 *      st5_stft_magnitude: reim fp32 [rows, 2*ldh] (real parts in columns [0,nbins), imaginary in [ldh, ldh+nbins)) ->
 *      mag fp32 [rows, ldh] = sqrt(re^2 + im^2), columns >= nbins zero.  st5_log10_floor: y = log10(max(x, floor)). */
int st5_stft_frames(const float* wav, float* out, int32_t B, int32_t S, int32_t n_fft, int32_t hop, void* stream);
int st5_stft_magnitude(const float* reim, float* mag, int64_t rows, int32_t nbins, int32_t ldh, void* stream);
int st5_log10_floor(const float* x, float* y, int64_t n, float floor_value, void* stream);
/* st5_stft_frames_rows: st5_stft_frames for B waveforms of DIFFERENT lengths in one launch (the per-item `logmelfilterbank` of
 * data/speech_to_speech_dataset.py:141-157 for a whole batch).  wav = device array of B base pointers (fp32 [len[b]]), len int32 [B],
 * frame_off int64 [B + 1] = running sum of L_b = 1 + len[b] / hop (frame_off[B] = total_frames).  out fp32 [total_frames, n_fft]
 * (16-byte aligned), item b's frames in rows [frame_off[b], frame_off[b + 1]), each centred and reflect-padded at the item's OWN
 * ends.  The caller guarantees len[b] > n_fft / 2 (the tables live on the device); n_fft % 4 == 0. */
int st5_stft_frames_rows(const float* const* wav, const int32_t* len, const int64_t* frame_off, float* out, int32_t B, int64_t total_frames,
                         int32_t n_fft, int32_t hop, void* stream);

/* ---- collation of the speech-pretraining batch on the device (data/speech_dataset.py:302-446 SpeechPretrainDataset.collater,
 *      collater_audio, crop_to_max_size, collater_frm_label; fairseq collate_tokens): every tensor of the batch is a RAGGED GATHER of
 *      the items' rows -- crop at a per-item start, thin out by a stride (the reduction factor), shift by one frame, pad to the
 *      longest.  st5_ragged_rows: out[b, t, 0:w] = src[b][(off[b] + t * step) * w + (0:w)] when t >= tmin and
 *      0 <= off[b] + t * step < hi[b], else the pad pattern; src = device array of B item base pointers, off / hi int32 [B], elements
 *      of es = 1, 4 or 8 bytes (copied as bits: fp32 wave / mel rows, int64 labels), pad_bits = the pad element's bit pattern.
 *      st5_tail_mask: out[b, t] = (t >= n[b]) ? 1 : 0 as uint8 (dtype_f32 = 0: padding_mask, :392-402) or fp32 (dtype_f32 = 1: the
 *      stop-token labels, :347-349).  The crop starts are drawn on the host from numpy's stream exactly as the reference draws them
 *      (one np.random.randint per item longer than the batch's audio size); speecht5_amd/collate.py drives both. */
int st5_ragged_rows(const void* const* src, const int32_t* off, const int32_t* hi, void* out, int32_t B, int32_t T, int32_t w, int32_t step,
                    int32_t tmin, int32_t es, uint64_t pad_bits, void* stream);
int st5_tail_mask(const int32_t* n, void* out, int32_t B, int32_t T, int32_t dtype_f32, void* stream);

/* ---- BatchNorm1d + tanh + dropout (+ residual) on channels-last rows: the non-GEMM part of the mel post-net
 *      (speech_decoder_postnet.py:39-51,65-70 = espnet Tacotron Postnet: 5 x [Conv1d k5 -> BatchNorm1d -> tanh -> dropout], the
 *      last block without tanh; after = before + postnet(before)).  x fp32 [rows, C] = the convolution GEMM's fp32 output
 *      (ST5_GEMM_OUT_F32), C % 4 == 0.  Training: batch statistics (fp64 partial sums), running_mean / running_var /
 *      num_batches_tracked updated like torch.nn.BatchNorm1d (momentum blend, unbiased variance); eval: running statistics.
 *      y = dropout(act((x - mean) * rstd * gamma + beta)) [+ residual], act in {ST5_ACT_NONE, ST5_ACT_TANH}; dropout element
 *      counters = row * C + c.  y: `dtype` elements, or fp32 when y_f32 (the block's fp32 `after` output); residual: `dtype`
 *      [rows, C].  Output row r goes to element offset (r / out_L) * out_bstride + (r % out_L) * C + out_off (out_L = 0: r * C)
 *      and `halo` rows in front of / behind every out_L-row batch block are zeroed: the next convolution's time-padded
 *      operand is written directly.  stats fp32 [2*C] (mean, rstd) is saved for the backward.  ws >= st5_batchnorm_ws_bytes(C). */
int64_t st5_batchnorm_ws_bytes(int32_t C);
int st5_batchnorm_act_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, float momentum, float eps, int32_t training, int32_t act,
                          float dropout_p, uint64_t seed, const void* residual, void* y, int32_t y_f32, float* stats, void* ws,
                          int64_t rows, int32_t C, int64_t out_L, int64_t out_bstride, int64_t out_off, int32_t halo, int dtype,
                          void* stream);
/* Backward: g = dropout_mask * dy * act'(.) with dy fp32 (the fp32 data gradient of the next convolution);
 * dgamma += sum g*xhat, dbeta += sum g (either may be NULL); dx (dtype, mapped / haloed like the forward's y) =
 * gamma * rstd * (g - mean(g) - xhat * mean(g * xhat)) for batch statistics, gamma * rstd * g for running statistics. */
int st5_batchnorm_act_bwd(const float* x, const float* dy, const float* stats, const float* gamma, const float* beta, float* dgamma,
                          float* dbeta, int32_t training, int32_t act, float dropout_p, uint64_t seed, void* dx, void* ws,
                          int64_t rows, int32_t C, int64_t out_L, int64_t out_bstride, int64_t out_off, int32_t halo, int dtype,
                          void* stream);
/* Live-frame variants for a FIXED-SHAPE batch (csrc/batchnorm_live_index.h): x is [B, Lx, C] and only the first *live rows of every
 * batch element exist in the batch the reference would have collated; `live` is ONE int32 cell in device memory, clamped by the
 * kernels to [0, Lx], so a captured launch serves every batch (the grid comes from the physical `rows` = B * Lx; nothing reads the
 * cell on the host).  Row r is live iff r % Lx < *live.  Statistics (and the running-statistics update, unbiased variance over
 * B * live - 1) range over the live rows; dead rows of y -- the next convolution's operand, or the fp32 output, the residual NOT
 * added -- and of dx are exact zeros; dy of a dead row counts as zero, so dgamma / dbeta take nothing from it.  training = 0: running
 * statistics plus the same zeroing.  Dropout counters stay the physical row * C + c: at *live == Lx every output is the bits of the
 * entry point above.  *live == 0: every output row zero, running statistics untouched.  out_L, when given, must equal Lx. */
int st5_batchnorm_act_fwd_live(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                               int64_t* num_batches_tracked, float momentum, float eps, int32_t training, int32_t act,
                               float dropout_p, uint64_t seed, const void* residual, void* y, int32_t y_f32, float* stats, void* ws,
                               int64_t rows, int32_t C, int64_t out_L, int64_t out_bstride, int64_t out_off, int32_t halo,
                               const int32_t* live, int64_t Lx, int dtype, void* stream);
int st5_batchnorm_act_bwd_live(const float* x, const float* dy, const float* stats, const float* gamma, const float* beta, float* dgamma,
                               float* dbeta, int32_t training, int32_t act, float dropout_p, uint64_t seed, void* dx, void* ws,
                               int64_t rows, int32_t C, int64_t out_L, int64_t out_bstride, int64_t out_off, int32_t halo,
                               const int32_t* live, int64_t Lx, int dtype, void* stream);
/* st5_pad_time with rows t >= *live of every batch element written as zeros (the post-net's first operand on a fixed-shape batch), and
 * x[b, t, :] = 0 for t >= *live on an fp32 [B, Lx, C] buffer (the post-net's input gradient); `live` as above. */
int st5_pad_time_live(const void* src, void* dst, int32_t B, int32_t T, int32_t C, int32_t pad_l, int32_t pad_r, const int32_t* live,
                      int dtype, void* stream);
int st5_zero_rows_live(float* x, int32_t B, int32_t Lx, int32_t C, const int32_t* live, void* stream);

/* ---- losses ---- */
/* Row-wise (label-smoothed) cross entropy on logits [rows, ld] (dtype, first V cols valid).
 * loss_sum[0] += sum_r w_r * ((1-eps)*nll_r + eps/V... ) following speech_to_text_loss.py:93-110;
 * target < 0 or == ignore_index rows are skipped.  Also writes dlogits = scale * dloss/dlogits. */
int st5_cross_entropy(const void* logits, const int32_t* target, float* loss_sum, float* nll_sum, void* dlogits,
                      int64_t rows, int32_t V, int64_t ld, float label_smoothing, int32_t ignore_index,
                      float grad_scale, int dtype, void* stream);

/* The same with per-row outputs instead of atomically accumulated sums: row_loss[r] (and row_nll[r] if given) = the row's
 * loss (0 for skipped rows); the caller sums them (deterministic).  This is what the criteria use
 * (speech_pretrain_criterion.py:98-141 NCE cross entropy, text_pretrain_criterion.py:56-60, speech_to_text_loss.py:93-110). */
int st5_cross_entropy_rows(const void* logits, const int32_t* target, float* row_loss, float* row_nll, void* dlogits,
                           int64_t rows, int32_t V, int64_t ld, float label_smoothing, int32_t ignore_index,
                           float grad_scale, int dtype, void* stream);

/* ---- optimizer (fairseq `adam`: decoupled weight decay; README.md:107-115 flags) ----
 * One fused pass over the flat fp32 buffers: g' = g * grad_scale * min(1, max_norm / (sqrt(*gnorm_sq) * grad_scale));
 * m,v update; p = p*(1 - lr*wd) - lr*sqrt(bc2)/bc1 * m / (sqrt(v) + eps) (fairseq/optim/adam.py: eps is not bias-corrected;
 * bc_i = 1 - beta_i^step).  gnorm_sq is a DEVICE scalar (may be NULL). */
int st5_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, const float* gnorm_sq, float max_norm, float grad_scale,
                  void* bf16_mirror /* optional bf16 [n]: receives the updated parameters in the compute dtype */, void* stream);
/* The same with the learning rate and the step count read from DEVICE memory (hyper_dev = {lr, step} as two floats; NULL =
 * the by-value arguments): the form a captured HIP graph replays -- its kernel arguments are frozen, the host rewrites the two
 * floats before every replay. */
int st5_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int32_t step, const float* gnorm_sq, float max_norm, float grad_scale, void* bf16_mirror,
                      const float* hyper_dev, void* stream);
/* ---- speech-decoder criterion (Tacotron2Loss with masking, text_to_speech_loss.py:263-345 + the label / length fix-ups of
 * :186-204) as one reduction + one gradient pass.  All tensors fp32 on the device; ys [B, >=L, C] and labels [B, >=L] with
 * their own batch strides (elements); olens int64 [B] (device) = the UNTRIMMED target lengths, r = reduction factor:
 * valid frames are t < olens - olens % r, the stop label of the last valid frame is 1.
 * fwd: out4 = {l1, mse, bce, n_frames}.   bwd: gradients of g_l1 * l1 + g_mse * mse + g_bce * bce (device scalars, NULL = 0)
 * w.r.t. after / before / logits (each may be NULL). */
int64_t st5_tacotron_loss_ws_bytes(void);
int st5_tacotron_loss_fwd(const float* after, const float* before, const float* logits, const float* ys, int64_t ys_bstride,
                          const float* labels, int64_t labels_bstride, const int64_t* olens, int32_t B, int32_t L, int32_t C, int32_t r,
                          float pos_weight, float* out4, void* ws, void* stream);
int st5_tacotron_loss_bwd(const float* after, const float* before, const float* logits, const float* ys, int64_t ys_bstride,
                          const float* labels, int64_t labels_bstride, const int64_t* olens, int32_t B, int32_t L, int32_t C, int32_t r,
                          float pos_weight, const float* out4, const float* g_l1, const float* g_mse, const float* g_bce, float* d_after,
                          float* d_before, float* d_logits, void* stream);
/* ---- CTC loss of the ASR criterion (speech_to_text_loss.py:301-337: F.ctc_loss(lprobs, flat targets, input_lengths,
 * target_lengths, blank, reduction="sum", zero_infinity), torch's own recursion since the reference turns cuDNN off) ----
 * lprobs [T, B, V] fp32 log-probabilities; targets int64, sentence b's labels at targets[target_offsets[b] ...
 * + target_lengths[b]) (lengths clamped to max_target_len); all index arrays on the device.
 * fwd: nll [B], loss[0] = sum_b nll_b (an impossible alignment counts 0 with zero_infinity); ws >= st5_ctc_loss_ws_bytes
 * keeps the alpha rows.  bwd: grad [T, B, V] = grad_out[0] * (exp(lprobs) - posterior) for t < input_lengths[b], else 0 --
 * the form torch's ctc_loss backward returns (the gradient w.r.t. the logits in front of the log-softmax; pushing it through
 * the log-softmax backward leaves it unchanged).  Both refuse (ST5_ERR_ARG, nothing launched) the same pairs: those with
 * (8 max_target_len + V + 12) * 4 bytes > 60 KiB of LDS, i.e. max_target_len > 1908 at V = 83. */
int64_t st5_ctc_loss_ws_bytes(int32_t T, int32_t B, int32_t max_target_len);
int st5_ctc_loss_fwd(const float* lprobs, const int64_t* targets, const int64_t* target_offsets, const int64_t* input_lengths,
                     const int64_t* target_lengths, int32_t T, int32_t B, int32_t V, int32_t max_target_len, int32_t blank,
                     int32_t zero_infinity, float* nll, float* loss, void* ws, void* stream);
int st5_ctc_loss_bwd(const float* lprobs, const int64_t* targets, const int64_t* target_offsets, const int64_t* input_lengths,
                     const int64_t* target_lengths, int32_t T, int32_t B, int32_t V, int32_t max_target_len, int32_t blank,
                     int32_t zero_infinity, const float* nll, const float* grad_out, const void* ws, float* grad, void* stream);
/* ---- CTC labels packed per row on the device (csrc/ctc_loss.hip, index arithmetic in csrc/ctc_pack_index.h).  The torch call site it
 * replaces is criterions.SpeechtoTextLoss.compute_loss_ctc's
 *     targets_flat = sample["target"].masked_select((target != pad) & (target != eos));  offsets = cumsum(lengths) - lengths
 * whose result has a data-dependent shape (a device-to-host read: no stream capture survives it).
 * target int64 [B, L] right-padded (label + </s>).  packed int64 [B, L]: row b holds the entries of target[b] that are neither `pad`
 * nor `eos`, in order, from column 0; the rest of the row is `pad` (every element is written).  offsets int64 [B] = b * L;
 * kept int64 [B] = kept entries per row; total int64 [1] = sum of kept, WRITTEN (never accumulated into: no memset in front of a
 * replayed launch).  (packed, offsets, lengths <= kept) with max_target_len = L is a legal input of st5_ctc_loss_fwd / _bwd: they
 * read targets[offsets[b] + i] for i < min(length_b, max_target_len) and assume nothing else about offsets.  One launch of one
 * workgroup, stable (ballot + prefix popcount per 64-column chunk), no atomics, no allocation, no host read: capturable.
 * B == 0, L == 0, negative sizes, a null pointer and packed == target return ST5_ERR_ARG with nothing launched. */
int st5_ctc_pack_rows(const int64_t* target, int64_t pad, int64_t eos, int32_t B, int32_t L, int64_t* packed, int64_t* offsets,
                      int64_t* kept, int64_t* total, void* stream);
/* ---- guided attention loss of the TTS criterion (text_to_speech_loss.py:370-427) ----
 * att [B, H, To, Ti] fp32 (the selected heads of the selected layers, concatenated), ilens / olens int64 [B] on the device.
 * fwd: out2 = {alpha * mean over (to < olen_b, ti < ilen_b) of (1 - exp(-(ti/ilen_b - to/olen_b)^2 / (2 sigma^2))) att, alpha / count}.
 * bwd: datt = grad_out[0] * out2[1] * weight inside the selection, 0 outside. */
int64_t st5_guided_attn_ws_bytes(void);
int st5_guided_attn_fwd(const float* att, const int64_t* ilens, const int64_t* olens, int32_t B, int32_t H, int32_t To, int32_t Ti,
                        float sigma, float alpha, float* out2, void* ws, void* stream);
int st5_guided_attn_bwd(const int64_t* ilens, const int64_t* olens, int32_t B, int32_t H, int32_t To, int32_t Ti, float sigma,
                        const float* out2, const float* grad_out, float* datt, void* stream);
/* ---- Gumbel vector quantizer + time-wise code / encoder-state mix (speecht5.py:95-107, 858-882; csrc/vq.hip) ----
 * logits, gumbel [N, G*V] fp32 (V <= 128); vars [G*V, Dg] fp32; enc / out [N, G*Dg] (dtype); mix_w [T] fp32 or NULL (rows are
 * (b, t) with t = n % T); tau by value or from tau_dev.  training = 0: hard arg-max of the logits, no noise.
 * fwd: out, idx [N, G] (code-book ROW g*V + v), avg [G][st5_vq_vpad()] (mean softmax, kept for bwd), perp2 = {code_perplexity,
 * prob_perplexity}.  bwd: dlogits [N, G*V] from dsel [N][dsel_ld >= G*vpad] (= dOut . vars_g^T per group, the caller's GEMM; NULL =
 * no code path), the upstream gradient of prob_perplexity (device scalar, NULL = 0); denc = (1 - w) dOut (NULL = skip). */
int64_t st5_vq_ws_bytes(void);
int32_t st5_vq_vpad(void);
int st5_vq_fwd(const float* logits, const float* gumbel, const float* vars, const void* enc, const float* mix_w, float tau, const float* tau_dev,
               int32_t training, void* out, int32_t* idx, float* avg, float* perp2, void* ws, int32_t N, int32_t G, int32_t V, int32_t Dg,
               int32_t T, int dtype, void* stream);
int st5_vq_bwd(const float* logits, const float* gumbel, const float* dsel, int32_t dsel_ld, const float* avg, const float* g_prob_perp,
               const void* dout, const float* mix_w, float tau, const float* tau_dev, int32_t training, float* dlogits, void* denc, int32_t N,
               int32_t G, int32_t V, int32_t Dg, int32_t T, int dtype, void* stream);
/* ---- HuBERT NCE head (speech_encoder_postnet.py:56-76), fp32 (csrc/nce.hip) ----
 * st5_norm_rows: y[r] = x[r] / max(|x[r]|, 1e-8) (x in `dtype`, y fp32), inv[r] = 1 / max(|x[r]|, 1e-8); st5_norm_rows_bwd: its
 * gradient dx (`dtype`; accumulate != 0: dx += ...).  st5_canon_rows: canon[c] = smallest c' whose row equals row c exactly.
 * st5_nce_logits: logits[s] = [sim[s, t_s], sim[s, :]] / temp with -inf where canon[c] == canon[t_s]; st5_nce_logits_bwd: dsim with row
 * stride dsim_ld >= V, its columns V..dsim_ld-1 written as zero (a ld that is a multiple of 4 makes dsim a GEMM operand for any V). */
int st5_norm_rows(const void* x, float* y, float* inv, int64_t rows, int32_t cols, int dtype, void* stream);
int st5_norm_rows_bwd(const float* y, const float* inv, const float* dy, void* dx, int64_t rows, int32_t cols, int32_t accumulate, int dtype,
                      void* stream);
int st5_canon_rows(const float* e, int32_t* canon, int32_t V, int32_t D, void* stream);
int st5_nce_logits(const float* sim, const int32_t* target, const int32_t* canon, float* logits, int64_t S, int32_t V, float temp, void* stream);
int st5_nce_logits_bwd(const float* dlogits, const int32_t* target, const int32_t* canon, float* dsim, int32_t dsim_ld, int64_t S, int32_t V,
                       float temp, void* stream);
/* A/B switch of the LayerNorm backward: upper bound of its block count (default 256). */
int st5_layernorm_set_max_blocks(int n);
/* ---- CTC prefix scoring for joint CTC / attention beam search (sequence_generator.py:273-418 calls espnet's
 * CTCPrefixScore per hypothesis on the host; in-tree copy Speech2C/speech2c/models/modules/ctc_prefix_score.py:10-112) ----
 * x: fp32 CTC log-posteriors [T, V] of ONE utterance (device).  A state is r[T][2] fp32 = log r_t^n, log r_t^b of a prefix.
 * st5_ctc_initial_state: the state of the empty prefix (:27-39).
 * st5_ctc_prefix_score: for nh hypotheses with states r_prev[nh][T][2], last label last[nh] and out_len labels after <sos>,
 * and nc candidate next labels per hypothesis cs[nh][nc] (int64): log_psi[nh][nc] = log prefix probability of each extension
 * (eos: probability that the prefix ends; blank: logzero = -1e10), r_new[nh][nc][T][2] = the extensions' states. */
int st5_ctc_initial_state(const float* x, int32_t T, int32_t V, int32_t blank, float* r, void* stream);
int st5_ctc_prefix_score(const float* x, int32_t T, int32_t V, int32_t blank, int32_t eos, const float* r_prev, const int64_t* last,
                         int32_t out_len, const int64_t* cs, int32_t nh, int32_t nc, float* log_psi, float* r_new, void* stream);
/* Rows form, for a batch: x [S][Tmax][V] right-padded in time, lens[S] int32 (device) the sentences' frame counts, sent[nh] int32
 * (device) the sentence of each hypothesis row.  Per (row, candidate) pair the arithmetic is st5_ctc_prefix_score's on
 * x[sent[h]][:lens[sent[h]]], bit for bit; no frame at or behind a sentence's count is read.  out_len may exceed a sentence's
 * frame count: eos scores logaddexp(r_prev[T_s - 1]), every other candidate logzero, the state is logzero.
 * st5_ctc_initial_state_rows: r[S][Tmax][2], logzero behind each sentence's frames.
 * st5_ctc_prefix_score_rows: r_prev[nh][Tmax][2]; log_psi[nh][nc]; r_new[nh][Tmax][nc][2] (candidates innermost), written for
 * frames < lens[sent[h]] only.
 * st5_ctc_select_rows: for n continued hypotheses, parent[n] (row of that launch) and token[n] (int64): state[n][Tmax][2] of the
 * extension (logzero behind the frames), prev_psi[n] its log_psi, known[n] (uint8) 0 when the token is not in cs[parent[n]]
 * (slot 0 is gathered then), sent_out[n] (int32, may be NULL) = sent[parent[n]]. */
int st5_ctc_initial_state_rows(const float* x, const int32_t* lens, int32_t S, int32_t Tmax, int32_t V, int32_t blank, float* r, void* stream);
int st5_ctc_prefix_score_rows(const float* x, const int32_t* lens, const int32_t* sent, int32_t S, int32_t Tmax, int32_t V, int32_t blank,
                              int32_t eos, const float* r_prev, const int64_t* last, int32_t out_len, const int64_t* cs, int32_t nh,
                              int32_t nc, float* log_psi, float* r_new, void* stream);
int st5_ctc_select_rows(const int32_t* lens, const int32_t* sent, int32_t S, int32_t Tmax, const int64_t* cs, int32_t nh, int32_t nc,
                        const float* log_psi, const float* r_new, const int64_t* parent, const int64_t* token, int32_t n, float* state,
                        float* prev_psi, uint8_t* known, int32_t* sent_out, void* stream);
/* ---- shallow-fusion LM decoding (csrc/lm_decode.hip): replaces the full-prefix LM call of ASR beam search,
 * SpeechT5/speecht5/sequence_generator.py:420-425 (lm_model(tokens[:, :step + 1]) + log_softmax + lprobs[:, :V_lm] += w * probs) ----
 * Slot cache of one layer: kv [rows_cap][Tmax][2C] (compute dtype, C = H * head_dim): slot (r, j) = [k | v] of hypothesis row r at
 * position j, written once.  Ancestry: anc [rows][anc_ld] int32, row r reads position j from slot (anc[r][j], j).
 * st5_lm_decode_attn (multihead_attention.py self-attention with incremental state, one query per row):
 * ctx[r][h*hd + i] = softmax_j(q[r] . k_j * hd^-0.5) v_j over positions j < t of head h, fp32 accumulation.  head_dim 64 or 80 and
 * H <= 64, else ST5_ERR_ARG.  q / kv 16-byte aligned, q_ld a multiple of 4 (fp32) / 8 (bf16), else ST5_ERR_ALIGN.  ws: fp32
 * workspace of st5_lm_decode_attn_ws_bytes(rows, t, H, head_dim) bytes (16-byte aligned; NULL when that is 0).  An anc entry
 * outside [0, rows_cap) gives NaN in that row's output. */
int64_t st5_lm_decode_attn_ws_bytes(int32_t rows, int32_t t, int32_t H, int32_t head_dim);
int st5_lm_decode_attn(const void* q, int64_t q_ld, const void* kv, int32_t rows_cap, int32_t Tmax, const int32_t* anc, int64_t anc_ld,
                       int32_t rows, int32_t t, int32_t H, int32_t head_dim, void* ctx, int64_t ctx_ld, float* ws, int dtype, void* stream);
/* st5_lm_reorder (the LM's share of reorder_incremental_state, sequence_generator.py:218-224): anc_new[r][j] = anc[order[r]][j] for
 * j < t and = r for t <= j < Tmax, r < rows_new; order int64 indexes the rows_old rows of anc (an entry outside gives -1 below t).
 * anc_new must not alias anc. */
int st5_lm_reorder(const int32_t* anc, int64_t anc_ld, const int64_t* order, int32_t rows_old, int32_t rows_new, int32_t t, int32_t Tmax,
                   int32_t* anc_new, int64_t new_ld, void* stream);
/* st5_lm_fuse_logprobs (sequence_generator.py:421-425): lprobs[r][c] += lm_weight * log_softmax(logits[r][:V_lm])[c] for c < V_lm;
 * lprobs fp32 [rows][lp_ld], logits in `dtype` [rows][lg_ld]; the log-softmax in fp32.  Columns >= V_lm are not touched. */
int st5_lm_fuse_logprobs(float* lprobs, int64_t lp_ld, const void* logits, int64_t lg_ld, int32_t rows, int32_t V_lm, float lm_weight,
                         int dtype, void* stream);
/* ---- Batched speech synthesis (T5TransformerModel.generate_speech_batch; csrc/tts_decode.hip) ----
 * st5_decode_cross_attn (multihead_attention.py:340-389 with one query per row b): ctx[b][h*64 + i] = softmax_j(q[b] . k_j * 64^-0.5) v_j
 * over the S encoder positions of row b, k_j = kv[(b*S + j)*kv_ld + k_off + h*64 ...], v_j at + H*64; a set byte kpm[b*S + j]
 * (uint8 [B][S], or NULL) excludes key j.  Scores, softmax and accumulation fp32; ctx [B][ctx_ld] and q [B][q_ld] in `dtype`.
 * probs (fp32, or NULL): probs[b*p_row + h*p_head + j] = the probability of key j (0 at an excluded key); nothing else of the
 * record is written.  head_dim 64 only and H <= 64, else ST5_ERR_ARG.  q / kv 16-byte aligned and q_ld, kv_ld, k_off multiples of
 * 4 (fp32) / 8 (bf16), else ST5_ERR_ALIGN.  ws: fp32 workspace of st5_decode_cross_attn_ws_bytes(B, S, H, head_dim) bytes (16-byte
 * aligned; NULL when that is 0). */
int64_t st5_decode_cross_attn_ws_bytes(int32_t B, int32_t S, int32_t H, int32_t head_dim);
int st5_decode_cross_attn(const void* q, int64_t q_ld, const void* kv, int64_t kv_ld, int64_t k_off, const uint8_t* kpm, int32_t B,
                          int32_t S, int32_t H, int32_t head_dim, void* ctx, int64_t ctx_ld, float* probs, int64_t p_row, int64_t p_head,
                          float* ws, int dtype, void* stream);
/* st5_tts_step_tail (speecht5.py:1233-1246 for B rows at decode step idx, 1 <= idx <= cap): y fp32 [B][y_ld] = r*odim features then r
 * stop logits.  For every row with done[b] == 0: probs[b][(idx-1)*r + k] = sigmoid(logit k), mel[b][(idx-1)*r + k][:] = feature frame
 * k, next[b][:] = frame r-1 (in `dtype`); the row stops (done[b] = 1, steps[b] = idx) when idx >= minlen[b] and (some probability
 * >= threshold or idx >= maxlen[b]).  Rows with done[b] != 0 are not written.  *active = rows with done == 0 afterwards.
 * mel [B][cap*r][odim], probs [B][cap*r] fp32; B <= 4096. */
int st5_tts_step_tail(const float* y, int64_t y_ld, int32_t B, int32_t r, int32_t odim, const int32_t* minlen, const int32_t* maxlen,
                      int32_t* done, int32_t* steps, int32_t idx, int32_t cap, float threshold, float* mel, float* probs, void* next,
                      int64_t next_ld, int32_t* active, int dtype, void* stream);
/* ---- Speaker-identification head (s2c, speaker_decoder_postnet.py; csrc/speaker_head.hip) ----
 * st5_angular_margin_fwd: out[b][v] = s * m(cos[b][v]) for v < V on fp32 cosine logits, with the margin only on column target[b]
 * (int32; -1 = no margin in that row, which is then only scaled).  mode ST5_MARGIN_AM (AngularMargin): s * (cos - m) on the target.
 * ST5_MARGIN_AAM / ST5_MARGIN_AAM_EASY (AdditiveAngularMargin): phi = cos*cos_m - sqrt(clamp(1 - cos^2, 0, 1))*sin_m on the target,
 * used where cos > th (else cos - mm), or with easy margin where cos > 0 (else cos); th = cos(pi - m), mm = sin(pi - m) * m.
 * out may be cos (in place).  st5_angular_margin_bwd: dcos = dy * d out / d cos, exactly; columns V..dcos_ld-1 of dcos are written
 * as zero.  Where the clamp is active (|cos| >= 1, the sine term is 0) its derivative is taken as 0: the target column's gradient
 * there is s * cos_m on the phi branch -- finite, where the reference's autograd gives inf or NaN.  B <= 65535. */
#define ST5_MARGIN_AM 0
#define ST5_MARGIN_AAM 1
#define ST5_MARGIN_AAM_EASY 2
int st5_angular_margin_fwd(const float* cos, int64_t ld, const int32_t* target, float* out, int64_t out_ld, int32_t B, int32_t V,
                           int32_t mode, float margin, float scale, void* stream);
int st5_angular_margin_bwd(const float* cos, int64_t ld, const int32_t* target, const float* dy, int64_t dy_ld, float* dcos,
                           int64_t dcos_ld, int32_t B, int32_t V, int32_t mode, float margin, float scale, void* stream);
/* st5_time_mean_fwd: y[b][c] = (1/T) sum_t x[t*t_stride + b*b_stride + c] over ALL T frames, padded ones included
 * (encoder_out.mean(1), speecht5.py:837-838); x in `dtype`, y fp32 [B, C]; compensated fp32 sums.  st5_time_mean_bwd: dx[t][b][c] =
 * dy[b][c] / T for every frame, dx time-major [T, B, C] contiguous in `dtype` (accumulate != 0: added to dx).  B <= 65535. */
int st5_time_mean_fwd(const void* x, int64_t t_stride, int64_t b_stride, int32_t T, int32_t B, int32_t C, float* y, int dtype,
                      void* stream);
int st5_time_mean_bwd(const float* dy, int32_t T, int32_t B, int32_t C, int32_t accumulate, void* dx, int dtype, void* stream);
/* ---- Speech enhancement output (s2s with --se-predict, SpeechT5/speecht5/models/speecht5.py:937-953; csrc/elementwise.hip) ----
 * The post-net's outputs `before` and `after` combined with the source features `src` (all fp32, n elements, same layout), both in
 * one launch.  ST5_SE_MASKING: y = sigmoid(x) * src; ST5_SE_DELTA: y = x - src (`target` returns the outputs as they are: no
 * kernel).  st5_se_predict_bwd: g = d * src * s * (1 - s) with s = sigmoid(x) recomputed from x (masking), g = d (delta); no gradient
 * goes to src (data).  Outputs do not alias inputs.  16-byte vectors when every pointer is 16-byte aligned, scalars otherwise. */
#define ST5_SE_MASKING 0
#define ST5_SE_DELTA 1
int st5_se_predict_fwd(const float* before, const float* after, const float* src, float* out_before, float* out_after, int64_t n,
                       int32_t mode, void* stream);
int st5_se_predict_bwd(const float* d_before, const float* d_after, const float* before, const float* after, const float* src,
                       float* g_before, float* g_after, int64_t n, int32_t mode, void* stream);
/* ... over TWO gradient buffers: the step uses g + g2 (g2 may be NULL); zero_grads != 0 leaves both buffers zeroed.  With
 * st5_sumsq_pair (sum of squares of x + y) for the clipping norm this replaces "g += g2", two fills and the plain step. */
int st5_adam_step_pair(float* p, float* g, float* g2, int32_t zero_grads, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int32_t step, const float* gnorm_sq, float max_norm, float grad_scale,
                       void* bf16_mirror, const float* hyper_dev, void* stream);
/* out[0] (+)= scale * sum((x + y)^2), fp32: bit-identical to st5_sumsq of the buffer x + y at the same alignment.  16-byte vectors when
 * x and y are 16-byte aligned, scalars otherwise (another summation order: see st5_sumsq). */
int st5_sumsq_pair(const float* x, const float* y, float* out, int64_t n, float scale, int32_t accumulate, void* stream);
/* ---- The Adam step behind a finite-gradient guard (ddp.FusedAdam(skip_nonfinite=True), update.PretrainUpdate(nonfinite="skip");
 * csrc/optim.hip) ----
 * st5_adam_step_pair with a verdict on the device: when gnorm_sq[0] is not finite -- NaN, inf, or a sum of finite squares that
 * overflowed fp32: !(gnorm_sq[0] <= FLT_MAX) -- the step is SKIPPED: p, m, v and bf16_mirror are neither read nor written (no weight
 * decay either), and with zero_grads != 0 the gradient buffers are left exact zeros, as an applied step leaves them.  Otherwise the
 * step is the one of st5_adam_step_pair, same bits, with the number of APPLIED steps in the bias corrections:
 * t_eff = t - skipped_before, t = `step` (hyper_dev[1] when hyper_dev is given), skipped_before = the skipped steps among 1 .. t - 1.
 * gnorm_sq is required (max_norm == 0 turns the clipping off, not the verdict).
 * guard: ST5_GUARD_CELLS int32 cells in device memory, all zero before the first step, owned by ONE optimizer:
 *   [ST5_GUARD_COUNT + 0], [ST5_GUARD_COUNT + 1]   the running count of skipped steps, double-buffered by the parity of t: the launch
 *                          of step t reads cell (t & 1) ^ 1 (what step t - 1 left) and one thread writes cell t & 1 -- no cell is
 *                          read and written in one launch.  REQUIRES t to advance by exactly one from launch to launch, starting at
 *                          1, all launches of one guard block on one stream (or otherwise ordered).  The count after step t is cell t & 1.
 *   [ST5_GUARD_SKIPPED]    1 when the most recent launch skipped its step, else 0
 *   [ST5_GUARD_STEP]       t of the most recent launch (what a host that kept count compares with its own)
 * The cells are written with ordinary stores by one thread and are visible to whatever follows the launch on its stream.
 * ST5_ERR_ARG: guard or gnorm_sq NULL (and what st5_adam_step_pair refuses). */
#define ST5_GUARD_COUNT 0
#define ST5_GUARD_SKIPPED 2
#define ST5_GUARD_STEP 3
#define ST5_GUARD_CELLS 4
int st5_adam_step_guard(float* p, float* g, float* g2, int32_t zero_grads, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                        float eps, float weight_decay, int32_t step, const float* gnorm_sq, float max_norm, float grad_scale,
                        void* bf16_mirror, const float* hyper_dev, int32_t* guard, void* stream);
/* Dropout seeds: every `seed` argument of this library may instead be a device pointer to the 64-bit seed, tagged with bit 63
 * (seed = (1 << 63) | pointer): the kernels then read the seed from memory (csrc/common.h resolve_seed).  Used by captured HIP
 * graphs, whose kernel arguments cannot change between replays. */
/* Batched bf16 matrix transposes in one launch.  jobs_dev: device array of {int64 src_off, int64 dst_off, int32 rows,
 * int32 cols, int32 tile0, int32 pad} sorted by tile0 (first 64x64 tile index of the job), offsets in elements into
 * src_flat / dst_flat; ntiles = total tile count.  Used for the transposed weight copies of the data-gradient GEMMs
 * (dX = dY.W as an NT product), refreshed once per optimizer step. */
int st5_multi_transpose_bf16(const void* src_flat, void* dst_flat, const void* jobs_dev, int32_t njobs, int32_t ntiles,
                             void* stream);

/* ---- Beam search over a slot cache (SequenceGenerator(decode="slots"); csrc/beam_decode.hip) ----
 * st5_beam_cross_attn (multihead_attention.py:340-389 with one query per hypothesis row r, rows = n_live * beam): row r belongs to live
 * sentence r / beam and reads the K/V block of original sentence s = sent[r / beam] (int32 [n_live]), of which all beam rows share
 * ONE copy: ctx[r][h*64 + i] = softmax_j(q[r] . k_j * 64^-0.5) v_j over the S encoder positions of sentence s,
 * k_j = kv[(s*S + j)*kv_ld + k_off + h*64 ...], v_j at + H*64 (one projection may hold all layers' K|V side by side); a set byte
 * kpm[s*S + j] (uint8 [n_sent][S], or NULL) excludes key j.  Scores, softmax and accumulation fp32; ctx [rows][ctx_ld] and
 * q [rows][q_ld] in `dtype`.  probs (fp32, or NULL): probs[r*p_row + h*p_head + j] = the probability of key j (exactly 0 at an
 * excluded key); nothing else of the record is written, and ctx is the same bits with and without it.  A K/V element is read once per
 * sentence and step (a workgroup covers up to 16 rows of a sentence; larger beams take further row groups).  The key-range split and
 * the reduction order are a function of (S, H, head_dim, dtype): a row's ctx bits do not depend on n_live, beam or the other rows.
 * No atomics.  head_dim 64 only and H <= 64, else ST5_ERR_ARG.  q / kv 16-byte aligned and q_ld, kv_ld, k_off multiples of 4 (fp32) /
 * 8 (bf16), else ST5_ERR_ALIGN.  A sent entry outside [0, n_sent) gives NaN in that sentence's rows (ctx and record) and is never
 * dereferenced.  ws: fp32 workspace of st5_beam_cross_attn_ws_bytes(rows, S, H, head_dim) bytes (16-byte aligned; NULL when 0). */
int64_t st5_beam_cross_attn_ws_bytes(int32_t rows, int32_t S, int32_t H, int32_t head_dim);
int st5_beam_cross_attn(const void* q, int64_t q_ld, const void* kv, int64_t kv_ld, int64_t k_off, const uint8_t* kpm, const int32_t* sent,
                        int32_t n_sent, int32_t n_live, int32_t beam, int32_t S, int32_t H, int32_t head_dim, void* ctx, int64_t ctx_ld,
                        float* probs, int64_t p_row, int64_t p_head, float* ws, int dtype, void* stream);

/* ---- the beam step on the device (csrc/beam_step.hip; SequenceGenerator(decode="device" / "graph"), sequence_generator.py:340-468 and
 * finalize_hypos :499-543 of this project's generator) ----
 * State, rows = n_sent * beam hypothesis rows, sentence s owns rows s*beam .. s*beam + beam - 1, never shrinks:
 *   counter int32[1]: the step (= input positions consumed so far);  tok int32 [rows][Tmax] / score fp32 [rows][Tmax] in SLOT layout:
 *   tok[r][j] = the token row r fed at position j (tok[.][0] = bos), score[r][j] = the cumulative score of the hypothesis that token
 *   closed (score[.][0] = 0); a hypothesis's history is read through the ancestry table, tokens[r][j] = tok[anc[r][j]][j];
 *   ignore uint8 [rows] (the generator's cands_to_ignore, by rank);  parent int32 [rows]: the row each continuing row came from;
 *   records: rec_tok int32 / rec_pos fp32 [rows][rec_ld] (hypothesis h of sentence s in row s*beam + h: tokens without bos, with the
 *   closing eos; per-position scores), rec_score fp32 [rows], rec_len int32 [rows], n_hyp int32 [n_sent], sent_done int32 [n_sent],
 *   n_finished int32 [1] (sentences finished, for the host to poll), ticket uint32 [1] (zero; the workgroups' arrival count).
 * st5_beam_step for step = *counter: log_softmax(logits / temperature) in fp32, the rules (eos -inf below min_len, NaN -> -inf, pad
 *   -inf, unk -= unk_penalty, never[c] != 0 -> -inf, at step >= max_len all but eos -inf; written to lprobs_out when given), top
 *   2 * beam of lprobs + score[.][step] per sentence (step 0: beam row 0 only) with the TIE RULE: higher score first, among equal
 *   scores (-inf included) the lower flat index beam_row * V + token; EOS / continuation / cands_to_ignore logic of the generator;
 *   finished hypotheses appended to the record while the sentence has fewer than `beam` and is not finished (score divided by
 *   len_div[step] when len_div is given: the host's fp32 table of (step + 1) ** len_penalty); a sentence is finished at `beam`
 *   hypotheses or at step == max_len; continuing rows get tok / score at position step + 1, parent and ignore (not at step ==
 *   max_len); the counter advances.  Nothing is written once the counter is past max_len.
 *   beam <= 32 and V - 1 >= 2 * beam, Tmax >= max_len + 1, rec_ld >= max_len + 1, else ST5_ERR_ARG.
 * st5_beam_reorder_dev, launched behind st5_beam_step: anc[r][j] = anc[parent[r]][j] for j < *counter, in place (parents lie inside
 *   the row's sentence; a parent outside gives -1); nothing when *counter > max_len.
 * st5_beam_embed_step: y[r] = emb_scale * table[tok[r][t]] + pos[clamp(t + pos_off)], t = clamp(*counter, 0, Tmax - 1): the text
 *   decoder pre-net's newest row (a token outside [0, V) gives NaN). */
int st5_beam_step(const float* logits, int64_t ld, float* lprobs_out, int64_t lp_ld, int32_t n_sent, int32_t beam, int32_t V,
                  float temperature, int32_t* tok, float* score, const int32_t* anc, int64_t anc_ld, int32_t Tmax, uint8_t* ignore,
                  int32_t* parent, int32_t* rec_tok, float* rec_pos, int64_t rec_ld, float* rec_score, int32_t* rec_len, int32_t* n_hyp,
                  int32_t* sent_done, int32_t* n_finished, uint32_t* ticket, int32_t* counter, const uint8_t* never, const float* len_div,
                  int32_t pad, int32_t unk, int32_t eos, float unk_penalty, int32_t min_len, int32_t max_len, void* stream);
int st5_beam_reorder_dev(int32_t* anc, int64_t anc_ld, const int32_t* parent, int32_t n_sent, int32_t beam, int32_t Tmax,
                         const int32_t* counter, int32_t max_len, void* stream);
/* st5_beam_step_logprobs: st5_beam_step on log-probabilities lp [rows][ld] instead of logits: the log-softmax is skipped (the rules'
 *   expression is evaluated with maximum 0, log-sum 0 and temperature 1, which returns lp[r][c] itself), everything else is
 *   st5_beam_step, the same kernel. */
int st5_beam_step_logprobs(const float* lp, int64_t ld, float* lprobs_out, int64_t lp_ld, int32_t n_sent, int32_t beam, int32_t V,
                           int32_t* tok, float* score, const int32_t* anc, int64_t anc_ld, int32_t Tmax, uint8_t* ignore, int32_t* parent,
                           int32_t* rec_tok, float* rec_pos, int64_t rec_ld, float* rec_score, int32_t* rec_len, int32_t* n_hyp,
                           int32_t* sent_done, int32_t* n_finished, uint32_t* ticket, int32_t* counter, const uint8_t* never,
                           const float* len_div, int32_t pad, int32_t unk, int32_t eos, float unk_penalty, int32_t min_len, int32_t max_len,
                           void* stream);
/* ---- the beam step PER SENTENCE (csrc/beam_step.hip, index arithmetic in csrc/beam_stream_index.h): the step of a beam-search stream
 * (SequenceGenerator.generate_stream, speecht5_amd/beam_stream.py), in which n_slots sentence slots of `beam` rows each are stepped by
 * one launch sequence and a slot whose sentence has finished is handed to the next waiting request between two groups of steps.
 * State, beside tok / score / anc / ignore / parent / the records of st5_beam_step (rows = n_slots * beam, Tmax >= cap + 2 columns,
 * rec_ld >= cap + 1, cap = the largest step limit):
 *   pos int32 [n_slots]: steps done by the slot's occupant;  maxlen int32 [n_slots]: its step limit (clamped into [0, cap] wherever it
 *   is read);  done int32 [n_slots]: 1 = finished or idle;  moved int32 [n_slots]: 1 = the last step advanced the slot;
 *   pos_rows int32 [rows]: pos_rows[r] = pos[r / beam], what st5_gemm_skinny_rows and st5_lm_decode_attn_rows take.
 *   There is no counter, no ticket and no n_finished: no workgroup reads another slot's pos, so the hand-off between two launches is
 *   the kernel boundary.  len_div is one fp32 table over 0 .. cap.
 * st5_beam_step_sents: workgroup s runs st5_beam_step's stages (the same kernel body, selection and tie rule) for step = pos[s] and
 *   max_len = maxlen[s].  A slot with done[s] != 0 (or pos[s] outside 0 .. maxlen[s]) writes moved[s] = 0 and nothing else, before any
 *   load of logits.  Otherwise, behind the stages: pos[s] = step + 1, the slot's pos_rows, moved[s] = 1; done[s] = 1 at `beam`
 *   hypotheses or at step == maxlen[s].
 * st5_beam_reorder_sents, launched behind it: st5_beam_reorder_dev for t = pos[s], only where moved[s] != 0.
 * st5_beam_embed_sents: st5_beam_embed_step at position pos[r / beam] + pos_off for row r; y holds n_slots * beam rows.
 * st5_beam_sents_admit: one launch for n_admit slots; desc int32 [n_admit][4] in device memory = (slot, max_len, frames, bos).  For the
 *   slot's rows: anc = identity over all Tmax columns, tok[r][0] = bos, score[r][0] = 0, ignore = 0, rec_len = 0; n_hyp[slot] = 0;
 *   pos = 0, pos_rows = 0, maxlen = clamp(max_len, 0, cap), done = 0; kpm uint8 [n_slots][S]: byte j of the slot = (j >= clamp(frames,
 *   0, S)).  A slot outside [0, n_slots) admits nothing; nothing of another slot is written (moved is left alone). */
int st5_beam_step_sents(const float* logits, int64_t ld, float* lprobs_out, int64_t lp_ld, int32_t n_slots, int32_t beam, int32_t V,
                        float temperature, int32_t* tok, float* score, const int32_t* anc, int64_t anc_ld, int32_t Tmax, uint8_t* ignore,
                        int32_t* parent, int32_t* rec_tok, float* rec_pos, int64_t rec_ld, float* rec_score, int32_t* rec_len,
                        int32_t* n_hyp, int32_t* pos, const int32_t* maxlen, int32_t* done, int32_t* moved, int32_t* pos_rows,
                        const uint8_t* never, const float* len_div, int32_t pad, int32_t unk, int32_t eos, float unk_penalty,
                        int32_t min_len, int32_t cap, void* stream);
int st5_beam_reorder_sents(int32_t* anc, int64_t anc_ld, const int32_t* parent, int32_t n_slots, int32_t beam, int32_t Tmax,
                           const int32_t* pos, const int32_t* maxlen, const int32_t* moved, int32_t cap, void* stream);
int st5_beam_embed_sents(const float* table, int32_t V, const int32_t* tok, int32_t Tmax, const int32_t* spos, int32_t n_slots, int32_t beam,
                         const float* pos, int32_t pos_rows, int32_t pos_off, float emb_scale, void* y, int64_t y_ld, int32_t cols, int dtype,
                         void* stream);
int st5_beam_sents_admit(const int32_t* desc, int32_t n_admit, int32_t n_slots, int32_t beam, int32_t cap, int32_t Tmax, int32_t* tok,
                         float* score, int32_t* anc, int64_t anc_ld, uint8_t* ignore, int32_t* n_hyp, int32_t* rec_len, int32_t* pos,
                         int32_t* pos_rows, int32_t* maxlen, int32_t* done, uint8_t* kpm, int32_t S, void* stream);
/* ---- joint CTC / attention scoring in the device-stepped beam search (csrc/beam_ctc.hip): the rows form of the CTC prefix scorer
 * behind the step counter of st5_beam_step.  rows = S * beam, row r belongs to sentence r / beam; x [S][Tfr][V], lens [S] as for
 * st5_ctc_prefix_score_rows; tok [rows][tok_ld] int32 is st5_beam_step's; nc candidates per row, nc <= 1024.  Buffers: state
 * [rows][Tfr][2], r_new [rows][Tfr][nc][2], log_psi [rows][nc], prev [rows], cs int32 [rows][nc], lp [rows][lp_ld], unknown int32 [1].
 * Nothing is written when the counter is outside the range given below.  Launch order inside a step: candidates, score, the beam
 * step on lp, select, st5_beam_reorder_dev.
 * st5_beam_ctc_candidates, step = *counter in [0, max_len]: lp[r][c] = (logits[r][c] / temperature - max) - log(sum), the unruled
 *   fp32 log-softmax with st5_beam_step's statistics; cs[r][0 .. nc) = the nc best tokens of lp[r], never[c] != 0 tokens and NaN
 *   counted as -inf, in rank order under the TIE RULE (higher value first, among equal values the lower token).  nc <= V.
 * st5_ctc_prefix_score_rows_dev, step = *counter in [0, max_len]: log_psi and r_new of st5_ctc_prefix_score_rows (bit for bit) for
 *   sent[r] = r / beam, out_len = step, last[r] = tok[r][step], then lp[r][cs[r][j]] = (float)(1 - ctc_weight) * lp[r][cs[r][j]] +
 *   (float)ctc_weight * (log_psi[r][j] - prev[r]), every operation rounded to fp32.  A candidate outside [0, V) gives log_psi NaN
 *   and leaves lp alone.  0 <= ctc_weight <= 1.
 * st5_ctc_select_dev, t = *counter in [1, max_len] (behind the beam step): row r continues row p = parent[r] with token tok[r][t];
 *   state[r] = the extension's state r_new[p][.][slot] (logzero at and behind the sentence's frames), prev[r] = log_psi[p][slot],
 *   slot = the token's position in cs[p].  A token outside cs[p]: slot 0 is gathered and *unknown = 1 (sticky), unless ignore[r] or
 *   sent_done[r / beam] is set.  A parent outside [0, rows): logzero state, prev NaN, *unknown = 1 under the same condition. */
int st5_beam_ctc_candidates(const float* logits, int64_t ld, int32_t rows, int32_t V, float temperature, const uint8_t* never,
                            const int32_t* counter, int32_t max_len, float* lp, int64_t lp_ld, int32_t* cs, int32_t nc, void* stream);
int st5_ctc_prefix_score_rows_dev(const float* x, const int32_t* lens, int32_t S, int32_t Tfr, int32_t V, int32_t blank, int32_t eos,
                                  int32_t beam, const float* r_prev, const int32_t* tok, int32_t tok_ld, const int32_t* counter,
                                  int32_t max_len, const int32_t* cs, int32_t nc, float* log_psi, float* r_new, const float* prev, float* lp,
                                  int64_t lp_ld, double ctc_weight, void* stream);
int st5_ctc_select_dev(const int32_t* lens, int32_t S, int32_t Tfr, int32_t beam, const int32_t* cs, int32_t nc, const float* log_psi,
                       const float* r_new, const int32_t* parent, const int32_t* tok, int32_t tok_ld, const uint8_t* ignore,
                       const int32_t* sent_done, const int32_t* counter, int32_t max_len, float* state, float* prev, int32_t* unknown,
                       void* stream);
int st5_beam_embed_step(const float* table, int32_t V, const int32_t* tok, int32_t Tmax, const int32_t* counter, const float* pos,
                        int32_t pos_rows, int32_t pos_off, float emb_scale, void* y, int64_t y_ld, int32_t rows, int32_t cols, int dtype,
                        void* stream);
/* ---- joint CTC / attention scoring PER SENTENCE SLOT (csrc/beam_ctc.hip, csrc/beam_step.hip; index arithmetic in
 * csrc/beam_stream_index.h): the CTC part of the step of a beam-search stream (generate_stream(joint_ctc=True),
 * speecht5_amd/beam_stream.py).  The same kernel bodies as the three kernels above under a template flag: slot s = r / beam reads
 * pos[s], maxlen[s] (clamped into [0, cap]), done[s], moved[s] of the st5_beam_step_sents state and frames[s] where the scalar forms
 * read *counter, max_len and lens.  rows = n_slots * beam; x [n_slots][S][V] fp32, the slot's posterior over frames[s] <= S frames;
 * frames int32 [n_slots]; state [rows][S][2], r_new [rows][S][nc][2], log_psi [rows][nc], prev [rows], cs int32 [rows][nc],
 * lp [rows][lp_ld], unknown int32 [n_slots].  Per (row, candidate) pair the bits are the scalar forms' at step pos[s].  None of these
 * writes done, pos or anything of another slot, and none reads another slot's CTC state.  Launch order inside a step: candidates_sents,
 * prefix_score_rows_sents, st5_beam_step_sents_logprobs on lp, select_sents, st5_beam_reorder_sents.
 * st5_beam_ctc_candidates_sents: st5_beam_ctc_candidates for step = pos[s].  A slot with done[s] != 0, or pos[s] outside
 *   0 .. maxlen[s], returns before its first load: its lp and cs rows are not written.
 * st5_ctc_prefix_score_rows_sents: st5_ctc_prefix_score_rows_dev under the same gate with T = clamp(frames[s], 0, S), out_len = pos[s],
 *   last[r] = tok[r][pos[s]].  The gate is uniform per workgroup.
 * st5_beam_step_sents_logprobs: st5_beam_step_sents on log-probabilities, as st5_beam_step_logprobs is st5_beam_step on them.
 * st5_ctc_select_sents, behind the beam step: acts only where moved[s] != 0 and 1 <= t = pos[s] <= maxlen[s]; st5_ctc_select_dev for the
 *   slot's rows with sent_done = done[s] as that step left it.  unknown[s] = 1 (sticky until the slot's next admission) when a row of
 *   slot s that still counts (ignore clear, done[s] clear) was continued by a token outside its parent's candidates, or has a parent
 *   outside its own slot (then: logzero state, prev NaN).
 * st5_ctc_sents_admit, behind st5_beam_sents_admit over the same descriptors (slot, max_len, frames, bos): frames[slot] =
 *   clamp(frames, 0, S); state of the slot's `beam` rows = st5_ctc_initial_state_rows' state of the slot's slice of x over those frames
 *   (the same arithmetic; logzero behind them); prev = 0 for the slot's rows; unknown[slot] = 0.  The slice of x is written by the
 *   caller in front of the launch.  A slot outside [0, n_slots) admits nothing; no other slot's bytes change. */
int st5_beam_ctc_candidates_sents(const float* logits, int64_t ld, int32_t n_slots, int32_t beam, int32_t V, float temperature,
                                  const uint8_t* never, const int32_t* pos, const int32_t* maxlen, const int32_t* done, int32_t cap,
                                  float* lp, int64_t lp_ld, int32_t* cs, int32_t nc, void* stream);
int st5_ctc_prefix_score_rows_sents(const float* x, const int32_t* frames, int32_t n_slots, int32_t S, int32_t V, int32_t blank, int32_t eos,
                                    int32_t beam, const float* r_prev, const int32_t* tok, int32_t tok_ld, const int32_t* pos,
                                    const int32_t* maxlen, const int32_t* done, int32_t cap, const int32_t* cs, int32_t nc, float* log_psi,
                                    float* r_new, const float* prev, float* lp, int64_t lp_ld, double ctc_weight, void* stream);
int st5_beam_step_sents_logprobs(const float* lp, int64_t ld, float* lprobs_out, int64_t lp_ld, int32_t n_slots, int32_t beam, int32_t V,
                                 int32_t* tok, float* score, const int32_t* anc, int64_t anc_ld, int32_t Tmax, uint8_t* ignore,
                                 int32_t* parent, int32_t* rec_tok, float* rec_pos, int64_t rec_ld, float* rec_score, int32_t* rec_len,
                                 int32_t* n_hyp, int32_t* pos, const int32_t* maxlen, int32_t* done, int32_t* moved, int32_t* pos_rows,
                                 const uint8_t* never, const float* len_div, int32_t pad, int32_t unk, int32_t eos, float unk_penalty,
                                 int32_t min_len, int32_t cap, void* stream);
int st5_ctc_select_sents(const int32_t* frames, int32_t n_slots, int32_t S, int32_t beam, const int32_t* cs, int32_t nc,
                         const float* log_psi, const float* r_new, const int32_t* parent, const int32_t* tok, int32_t tok_ld,
                         const uint8_t* ignore, const int32_t* pos, const int32_t* maxlen, const int32_t* done, const int32_t* moved,
                         int32_t cap, float* state, float* prev, int32_t* unknown, void* stream);
int st5_ctc_sents_admit(const int32_t* desc, int32_t n_admit, int32_t n_slots, int32_t beam, const float* x, int32_t S, int32_t V,
                        int32_t blank, int32_t* frames, float* state, float* prev, int32_t* unknown, void* stream);
/* ---- shallow fusion of a language model in the device-stepped beam search (csrc/beam_lm.hip), step = *counter in [0, max_len], nothing
 * is written outside it.  lm_logits [rows][lm_ld] in `lm_dtype` (ST5_F32 / ST5_BF16), V_lm <= V; lp [rows][lp_ld] fp32.
 * st5_beam_lm_logprobs, logits != NULL: lp[r][c] = (logits[r][c] / temperature - max) - log(sum), st5_beam_ctc_candidates' lp (the
 *   same statistics and bits), then for c < V_lm: lp[r][c] += lm_weight * ((lm_logits[r][c] - max_lm) - log(sum_lm)); the beam step on
 *   log-probabilities follows.  logits == NULL: the LM term alone is added into lp in place (the CTC-mixed log-probabilities; behind
 *   st5_ctc_prefix_score_rows_dev, in front of st5_beam_step_logprobs).  The product and the sum are each rounded to fp32 (torch's
 *   lprobs[:, :V_lm] += lm_weight * log_softmax); columns V_lm .. V - 1 get no LM term; -inf stays -inf. */
int st5_beam_lm_logprobs(const float* logits, int64_t ld, int32_t rows, int32_t V, float temperature, const void* lm_logits, int64_t lm_ld,
                         int32_t V_lm, float lm_weight, int lm_dtype, const int32_t* counter, int32_t max_len, float* lp, int64_t lp_ld,
                         void* stream);
/* st5_beam_lm_logprobs_sents: st5_beam_lm_logprobs PER SENTENCE SLOT (the step of a beam-search stream with an LM,
 * speecht5_amd/beam_stream.py), the same kernel body under a template flag.  rows = n_slots * beam; row r belongs to slot s = r / beam
 * and is scored at step = pos[s] under maxlen[s] (clamped into [0, cap]) of the st5_beam_step_sents state.  A slot with done[s] != 0,
 * or pos[s] outside 0 .. maxlen[s], returns before its first load: its rows of lp are not written.  Both forms (logits != NULL and
 * in place); per live row the bits are st5_beam_lm_logprobs' at that step.  n_slots <= 65535, beam <= 32.  Launched behind the LM's
 * per-row step, in front of st5_beam_step_sents_logprobs; with CTC behind st5_ctc_prefix_score_rows_sents. */
int st5_beam_lm_logprobs_sents(const float* logits, int64_t ld, int32_t n_slots, int32_t beam, int32_t V, float temperature,
                               const void* lm_logits, int64_t lm_ld, int32_t V_lm, float lm_weight, int lm_dtype, const int32_t* pos,
                               const int32_t* maxlen, const int32_t* done, int32_t cap, float* lp, int64_t lp_ld, void* stream);

/* Skinny-M GEMM of the decode loops (csrc/decode_gemm.hip): out[m, n] = epilogue(sum_k x[m, k] * w[n, k] + bias[n]) for 1 <= M <= 32,
 * w in nn.Linear layout [N, K] (stacked weights are one [sum N_i, K] matrix), x / w / res in `dtype`, fp32 accumulation.  Weight-streaming:
 * every weight byte is read once; row m of out depends on row m of x only (same bits for any M and any other rows); the reduction order
 * is a function of (N, K, dtype); no atomics.  Epilogue in st5_gemm's order: + bias (fp32 [N] or NULL), act (ST5 ACT_NONE / GELU / RELU /
 * TANH), dropout (p in [0, 1), `seed` by value or tagged seed slot, element index (row0 + m) * N + n), + res (or NULL); out in `dtype`,
 * or fp32 when out_f32 != 0.  step != NULL: the output base is out + clamp(*step, 0, step_cap - 1) * step_stride elements (device-side
 * slot index of a decode step).  ws: fp32 workspace of st5_gemm_skinny_ws_bytes(N, K) bytes (0: none needed).  M > 32 or an unknown
 * act: ST5_ERR_ARG; x / w not 16-byte aligned, or x_ld / w_ld / K not a multiple of 16 bytes of elements: ST5_ERR_ALIGN. */
int64_t st5_gemm_skinny_ws_bytes(int32_t N, int32_t K);
int st5_gemm_skinny(const void* x, int64_t x_ld, const void* w, int64_t w_ld, const float* bias, const void* res, int64_t res_ld, void* out,
                    int64_t out_ld, int32_t M, int32_t N, int32_t K, int32_t act, float dropout_p, uint64_t seed, int32_t row0,
                    int32_t out_f32, const int32_t* step, int64_t step_stride, int32_t step_cap, float* ws, int dtype, void* stream);
/* Decode kernels with the step index in device memory (a decode step captured into a HIP graph cannot carry a host-side index).
 * st5_lm_decode_attn_dev: st5_lm_decode_attn with t = clamp(*step + t_add, 1, t_max); grid and ws (st5_lm_decode_attn_ws_bytes(rows,
 * t_max, ...)) are sized for t_max, key ranges past t exit at once, and the result is bit-equal to st5_lm_decode_attn(t).
 * st5_decode_cross_attn_step: st5_decode_cross_attn whose record column is clamp(*step, 0, cap - 1): probs points at column 0 and
 * p_col is the column stride (p_head >= cap * p_col).
 * st5_tts_step_tail_dev: st5_tts_step_tail for idx = *counter + 1, then *counter = idx; with *counter outside [0, cap) nothing is
 * written.  n_seeds > 0: seed_slots[k] = seed_table[idx * n_seeds + k] for the NEXT step (idx < cap), the per-step dropout seeds of the
 * pre-net.  st5_tts_pe_add_step: y[b, :C] = x[b, :C] + alpha[0] * table[clamp(*step, 0, table_rows - 1), :C]. */
int st5_lm_decode_attn_dev(const void* q, int64_t q_ld, const void* kv, int32_t rows_cap, int32_t Tmax, const int32_t* anc, int64_t anc_ld,
                           int32_t rows, const int32_t* step, int32_t t_add, int32_t t_max, int32_t H, int32_t head_dim, void* ctx,
                           int64_t ctx_ld, float* ws, int dtype, void* stream);
int st5_decode_cross_attn_step(const void* q, int64_t q_ld, const void* kv, int64_t kv_ld, int64_t k_off, const uint8_t* kpm, int32_t B,
                               int32_t S, int32_t H, int32_t head_dim, void* ctx, int64_t ctx_ld, float* probs, int64_t p_row,
                               int64_t p_head, int64_t p_col, const int32_t* step, int32_t cap, float* ws, int dtype, void* stream);
int st5_tts_step_tail_dev(const float* y, int64_t y_ld, int32_t B, int32_t r, int32_t odim, const int32_t* minlen, const int32_t* maxlen,
                          int32_t* done, int32_t* steps, int32_t* counter, int32_t cap, float threshold, float* mel, float* probs, void* next,
                          int64_t next_ld, int32_t* active, const uint64_t* seed_table, uint64_t* seed_slots, int32_t n_seeds, int dtype,
                          void* stream);
int st5_tts_pe_add_step(const void* x, int64_t x_ld, const float* table, int32_t table_rows, const float* alpha, const int32_t* step,
                        void* y, int64_t y_ld, int32_t B, int32_t C, int dtype, void* stream);
/* Decode kernels with ONE POSITION PER ROW (the synthesis stream, speecht5_amd/tts_stream.py: a fixed set of rows whose finished rows
 * are handed to waiting utterances).  pos int32 [rows] in device memory = steps completed by the current occupant of each row.  Every
 * value read from pos is clamped or range-checked before it enters an address: a wrong pos gives a wrong row, never a store out of
 * bounds.  Each form runs the kernels of its scalar form with the position looked up per row (once per workgroup, wave-uniform, or in
 * the epilogue behind the product), so row b's bits are those of the scalar form run at the same row count with the step pos[b].
 * st5_gemm_skinny_rows: st5_gemm_skinny whose row m lands at out + clamp(step_rows[row0 + m], 0, step_cap - 1) * step_stride +
 *   m * out_ld (row chunks of 32 index step_rows through row0).  step_rows is required.
 * st5_lm_decode_attn_rows: st5_lm_decode_attn_dev with t_b = clamp(pos[b] + t_add, 1, t_max) per row; grid and ws as for t_max (a row's
 *   partial states sit at the grid's split stride in ws, so rows with different split counts never share a cell).
 * st5_decode_cross_attn_rows: st5_decode_cross_attn_step whose record column of row b is clamp(pos[b], 0, cap - 1).  S is the buffers'
 *   capacity; a row's own encoder length is expressed by kpm.
 * st5_tts_pe_add_rows: st5_tts_pe_add_step with the positional row table[clamp(pos[b], 0, table_rows - 1)] per row.
 * st5_tts_step_tail_rows: a row with done[b] == 0 and pos[b] in [0, cap) runs st5_tts_step_tail's row at idx_b = pos[b] + 1 (frames,
 *   probabilities, next, the stop test against minlen[b] / maxlen[b]: done[b] = 1, steps[b] = idx_b) and pos[b] = idx_b; any other row
 *   writes nothing and does not advance.  *active = the rows that ran this step and did not stop in it.  tick (int32 [1], or NULL):
 *   *tick = (*tick + 1) mod table_rows (a value outside [0, table_rows) counts as -1), and with n_seeds > 0 seed_slots[k] =
 *   seed_table[*tick * n_seeds + k]: the next tick's pre-net dropout seeds.  The host refills the table between groups of ticks, so a
 *   stream of any length draws fresh seeds in tick order.  B <= 4096.
 * st5_tts_rows_admit: one launch for the n_admit rows handed to new utterances; desc int32 [n_admit][4] in device memory =
 *   {row b, encoder length T_b, minlen, maxlen}, rows distinct.  Per entry: pos[b] = done[b] = steps[b] = 0, minlen[b], maxlen[b],
 *   next[b][:odim] = 0, kpm[b][j] = (j >= clamp(T_b, 0, S)) for all j < S, and with spk_src (compute dtype [n_admit][spk_src_ld])
 *   spk_dst[b * spk_dst_ld + d] = spk_src[i * spk_src_ld + d] for d < D (the normalised speaker embedding into its columns of the
 *   speaker-integration input; spk_dst points at the first such column of row 0).  An entry whose row is outside [0, rows) admits
 *   nothing.  n_admit == 0: nothing is launched. */
int st5_gemm_skinny_rows(const void* x, int64_t x_ld, const void* w, int64_t w_ld, const float* bias, const void* res, int64_t res_ld,
                         void* out, int64_t out_ld, int32_t M, int32_t N, int32_t K, int32_t act, float dropout_p, uint64_t seed,
                         int32_t row0, int32_t out_f32, const int32_t* step_rows, int64_t step_stride, int32_t step_cap, float* ws,
                         int dtype, void* stream);
int st5_lm_decode_attn_rows(const void* q, int64_t q_ld, const void* kv, int32_t rows_cap, int32_t Tmax, const int32_t* anc, int64_t anc_ld,
                            int32_t rows, const int32_t* pos, int32_t t_add, int32_t t_max, int32_t H, int32_t head_dim, void* ctx,
                            int64_t ctx_ld, float* ws, int dtype, void* stream);
int st5_decode_cross_attn_rows(const void* q, int64_t q_ld, const void* kv, int64_t kv_ld, int64_t k_off, const uint8_t* kpm, int32_t B,
                               int32_t S, int32_t H, int32_t head_dim, void* ctx, int64_t ctx_ld, float* probs, int64_t p_row,
                               int64_t p_head, int64_t p_col, const int32_t* pos, int32_t cap, float* ws, int dtype, void* stream);
int st5_tts_pe_add_rows(const void* x, int64_t x_ld, const float* table, int32_t table_rows, const float* alpha, const int32_t* pos,
                        void* y, int64_t y_ld, int32_t B, int32_t C, int dtype, void* stream);
int st5_tts_step_tail_rows(const float* y, int64_t y_ld, int32_t B, int32_t r, int32_t odim, const int32_t* minlen, const int32_t* maxlen,
                           int32_t* done, int32_t* steps, int32_t* pos, int32_t cap, float threshold, float* mel, float* probs, void* next,
                           int64_t next_ld, int32_t* active, int32_t* tick, const uint64_t* seed_table, int32_t table_rows,
                           uint64_t* seed_slots, int32_t n_seeds, int dtype, void* stream);
int st5_tts_rows_admit(const int32_t* desc, int32_t n_admit, int32_t rows, int32_t* pos, int32_t* done, int32_t* steps, int32_t* minlen,
                       int32_t* maxlen, void* next, int64_t next_ld, int32_t odim, uint8_t* kpm, int32_t S, const void* spk_src,
                       int64_t spk_src_ld, void* spk_dst, int64_t spk_dst_ld, int32_t D, int dtype, void* stream);

/* ---- validation UER / WER of the ASR criterion (speech_to_text_loss.py:232-297), csrc/asr_metrics.hip ----
 * All arrays on the device; rows are int32 [B, L] with int32 lengths [B] unless said otherwise.  Every length is clamped to its row
 * inside the kernels; token VALUES are compared or range-checked, never trusted as indices.
 * st5_ctc_greedy_rows: lprobs [T, B, V] fp32 (st5_ctc_loss_fwd's layout), input_lengths [B] int64.  Per frame t < clamp(len_b, 0, T)
 *   the argmax over V by torch's CPU rule (lowest index among equal maxima; a NaN beats every number, the first NaN wins), then
 *   unique_consecutive, then blanks dropped: frame t is kept iff best[t] != blank and (t == 0 or best[t] != best[t - 1]).
 *   pred [B, T] (-1 behind pred_len[b]), pred_len [B]; best_ws [B, T] int32 workspace.
 * st5_tokens_to_words: the sentence's bytes = concatenation of the table's byte strings of its tokens (table_offsets [V + 1] into
 *   table_bytes [table_nbytes], no string longer than max_symbol_bytes), written to bytes [B, cap], cap = L * max_symbol_bytes;
 *   a word is a maximal run of bytes other than 0x20: word_start / word_len [B, word_cap], word_cap = (cap + 1) / 2, n_words [B].
 *   A token outside [0, V) contributes no bytes and sets err_flag[0] = 1 (the caller zeroes it).
 * st5_word_ids: p_ids [B, p_word_cap], t_ids [B, t_word_cap] with id(predicted word) == id(target word) iff their bytes are equal
 *   (lengths compared first), id(target word) == id(target word) iff their bytes are equal.
 * st5_edit_distance_rows: dist[b] = unit-cost Levenshtein distance of a[b][:a_len[b]] and b[b][:b_len[b]]; anti-diagonals, three
 *   rotating diagonals of min(La, Lb) + 1 ints in LDS.  min(La, Lb) > 4095 is refused (ST5_ERR_ARG, nothing launched). */
int st5_ctc_greedy_rows(const float* lprobs, const int64_t* input_lengths, int32_t T, int32_t B, int32_t V, int32_t blank,
                        int32_t* best_ws, int32_t* pred, int32_t* pred_len, void* stream);
int st5_tokens_to_words(const int32_t* tokens, const int32_t* len, int32_t B, int32_t L, const int32_t* table_offsets,
                        const uint8_t* table_bytes, int32_t V, int32_t table_nbytes, int32_t max_symbol_bytes, int32_t cap,
                        int32_t word_cap, uint8_t* bytes, int32_t* word_start, int32_t* word_len, int32_t* n_words, int32_t* err_flag,
                        void* stream);
int st5_word_ids(const uint8_t* p_bytes, const int32_t* p_start, const int32_t* p_len, const int32_t* p_n, int32_t p_cap,
                 int32_t p_word_cap, const uint8_t* t_bytes, const int32_t* t_start, const int32_t* t_len, const int32_t* t_n,
                 int32_t t_cap, int32_t t_word_cap, int32_t B, int32_t* p_ids, int32_t* t_ids, void* stream);
int st5_edit_distance_rows(const int32_t* a, const int32_t* a_len, int32_t La, const int32_t* b, const int32_t* b_len, int32_t Lb,
                           int32_t B, int32_t* dist, void* stream);

/* ---- batch load: the tensor leaves of an update's micro-batches copied into the captured step's static inputs by one launch
 *      (csrc/batch_load.hip, index arithmetic in csrc/batch_load_index.h; speecht5_amd/graph.py BatchFeed).
 * All four arrays live in DEVICE memory.  dst [n_leaves] (destination addresses), bytes [n_leaves] (byte counts >= 0) and
 *   prefix [n_leaves + 1] (exclusive prefix of ceil(bytes / 256), prefix[0] = 0, prefix[n_leaves] = total_chunks) are written once by
 *   the caller and constant afterwards; src [n_leaves] (source addresses) is the only thing that changes between launches.
 * Contract: the kernel trusts the table.  The caller guarantees that every source and destination is a device allocation of at
 *   least bytes[i] bytes that stays alive until the launch has completed, that no destination overlaps another destination or any
 *   source, and that prefix and total_chunks follow from bytes as stated; n_leaves and total_chunks are launch arguments, and no
 *   other size is read from anything the incoming batch wrote.  A leaf of zero bytes has no chunk and its addresses are never read.
 * Any alignment is accepted: a lane moves 16 bytes at once when its source and destination are both 16-byte aligned, else (and in
 *   a leaf's tail) byte by byte.  No atomics, no LDS.  total_chunks == 0: nothing is launched.  n_leaves < 0, total_chunks < 0, a
 *   NULL array with work to do: ST5_ERR_ARG. */
int st5_batch_load(const void* const* src, const void* const* dst, const int64_t* bytes, const int64_t* prefix, int32_t n_leaves,
                   int64_t total_chunks, void* stream);

/* ---- training statistics: the logged scalars of one update copied into a row of a device ring by one launch, the last of the
 *      update (csrc/train_stats.hip, arithmetic in csrc/train_stats_index.h; speecht5_amd/train_stats.py StatsRecorder).
 * Replaces, on the replayed path, the trainer's `.item()` per logged scalar (fairseq Trainer.train_step -> reduce_metrics reads every
 *   entry of the criterion's logging output on the host; under graph replay that Python does not run and the scalars live in the
 *   graph's private pool).
 * All four arrays live in DEVICE memory.  src [n_cells]: addresses of one-element device tensors; types [n_cells]: int32 type codes
 *   (0 fp32, 1 fp64, 2 bf16, 3 fp16, 4 int64, 5 int32, 6 uint8 / bool; any other code: the cell is written as 0 and nothing is read);
 *   ring [rows, 1 + n_cells]: 8-byte cells; counter [1]: int64, the number of updates recorded so far.
 * Row counter % rows: cell 0 = counter (the stamp), cell 1 + i = the scalar at src[i], floating types widened to fp64 (exact for
 *   fp32, bf16, fp16; a NaN stays a NaN), integer and bool types to int64.  Then counter becomes counter + 1.  Launches on one stream
 *   are ordered, so consecutive launches fill consecutive rows; no other row and no byte outside ring and counter is written.
 * Contract: the kernel trusts the arrays.  The caller guarantees that every source is a live, naturally aligned device scalar of its
 *   type until the launch has completed.  One workgroup, no atomics, no LDS.  n_cells < 1, n_cells > 1024, rows < 1 or a NULL array:
 *   ST5_ERR_ARG, nothing launched. */
int st5_stats_record(const void* const* src, const int32_t* types, void* ring, int64_t* counter, int32_t rows, int32_t n_cells,
                     void* stream);

/* ---- state digest: one 64-bit digest per segment of a set of device segments, the check of a checkpoint's bytes on their way
 *      from the device to a file (csrc/state_digest.hip, arithmetic in csrc/state_digest_index.h; speecht5_amd/checkpoint.py).
 * Definition, all arithmetic mod 2^64, for a segment of n bytes: w_i its little-endian 8-byte words (the last one zero-padded),
 *   digest = h((sum over i of h(w_i + (i + 1) * 0x9E3779B97F4A7C15)) + n), h the splitmix64 finaliser.  A wrapped integer sum: the
 *   result does not depend on the order of the additions, so two calls on the same bytes always give the same cells.
 * All four arrays live in DEVICE memory.  seg [n_seg] (segment addresses), bytes [n_seg] (byte counts >= 0), prefix [n_seg + 1]
 *   (exclusive prefix of ceil(bytes / 256), prefix[0] = 0, prefix[n_seg] = total_chunks), out [n_seg] (the digests, 8-byte cells).
 * Contract: read-only on the segments; the kernel trusts the table.  The caller guarantees that every segment is a device allocation
 *   of at least bytes[i] bytes that stays alive and unwritten until the call's work has completed, and that prefix and total_chunks
 *   follow from bytes as stated.  Any byte alignment of a segment is accepted: a lane reads 16 bytes at once when the segment's
 *   base is 16-byte aligned, else (and in a segment's tail) byte by byte.  A segment of zero bytes has no chunk, its address is never
 *   read and its digest is h(0).  The cells need no preparation: the call clears them itself (a memset node), accumulates with
 *   64-bit integer atomics and finishes them with a second small kernel, all on `stream`; no allocation, no host synchronisation,
 *   capturable.  No LDS, no barrier.  n_seg < 0, total_chunks < 0, n_seg == 0 with total_chunks > 0, a NULL array with n_seg > 0:
 *   ST5_ERR_ARG, nothing enqueued.  n_seg == 0 and total_chunks == 0: nothing to do, ST5_OK. */
int st5_state_digest(const void* const* seg, const int64_t* bytes, const int64_t* prefix, int32_t n_seg, int64_t total_chunks,
                     uint64_t* out, void* stream);

const char* st5_version(void);

#ifdef __cplusplus
}
#endif
#endif
