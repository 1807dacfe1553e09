/* carel_hip.h -- C ABI of libcarel_hip.so, the MI355X (gfx950) implementation of the CAREL-VAE training
 * hot path (reference: drl_classifier_ec_mmd_final_mul.py; "ref:" line numbers below are into that file
 * of tk1363704/CAREL-VAE unless another file is named).
 *
 * The reference has no FFI of its own (it is 100 % Python); the boundary a maintainer binds is the set
 * of torch / transformers calls on the step path.  Each entry point names the reference call it replaces.
 * See INTEGRATION.md for the ctypes stub that goes into the reference's script.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch tensor.data_ptr()) unless marked "host";
 *   - plain-old-data argument structs, no torch types; row-major tensors;
 *   - every call only ENQUEUES work on `stream` (void* = hipStream_t): no device allocation, no host sync.  Process-wide
 *     state the library does keep: the thread-local error string; per device, three library-owned streams and ten events
 *     created on first use (overlap_wgrad / forward chains, see carel_encoder_args); a 20-KiB table of gelu / gelu' by bf16 input in
 *     device memory, filled by carel_init (the one call that synchronises the device), immutable afterwards; the carel_profile_gemm
 *     event log (measurement aid).  None of it changes results.  The product library has NO tuning hooks and no other mutable
 *     process-wide state (ABI 7): carel_gemm_set_variant and the kernels that were built, measured and not adopted live in the
 *     EXPERIMENTS build only (libcarel_hip_exp.so, -DCAREL_EXPERIMENTS; include/carel_hip_experiments.h);
 *   - return 0 on success, a negative CAREL_ERR_* otherwise; carel_last_error() gives the message;
 *   - "bf16" = raw bfloat16 bits (uint16_t); "f32" = IEEE float.
 */
#ifndef CAREL_HIP_H
#define CAREL_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CAREL_OK 0
#define CAREL_ERR_ARG (-1)    /* null pointer / inconsistent arguments */
#define CAREL_ERR_SHAPE (-2)  /* shape not supported by the kernels     */
#define CAREL_ERR_HIP (-3)    /* a HIP runtime call or launch failed    */

/* ABI version of this header; carel_abi_version() must return the same number. */
#define CAREL_ABI_VERSION 9

int carel_abi_version(void);
/* Checks that `device` is a gfx950 part and fills the library's only per-device state, immutable afterwards: the 20-KiB GELU table of
 * the fused FFN1 epilogue (one small kernel + one hipDeviceSynchronize -- the ONLY host synchronisation in the library; no other call
 * synchronises).  Must be called once per device per process before the first carel_gemm_bf16 / carel_encoder_* call on it (those
 * fail with CAREL_ERR_ARG otherwise); calling it again is a no-op.  The host mirror does it when a model is moved to the device
 * (carel_vae_amd._lib.ensure_init).  ref: `model.to(device)` :932 */
int carel_init(int device);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* carel_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Counter-based dropout.  With j = idx + idx_offset and h = mix32((j >> 1) ^ mix32(seed + site*0x9E3779B9)), element j is kept iff
 * the 16-bit half (j & 1) of h is >= floor(p * 2^32) >> 16 (two consecutive elements share one 32-bit hash: the attention kernels take
 * 25 M decisions per layer and direction); kept values are scaled by 1/(1-p).  p <= 0 disables.  `site` numbers the
 * dropout layer (0 embeddings; 1+3l attention probabilities, 2+3l attention-output, 3+3l FFN-output of
 * encoder layer l; 100/101/102 the three classifier-input dropouts, ref :468 :485 :503).
 * Replaces nn.Dropout inside HF BertEmbeddings/BertSelfAttention/BertSelfOutput/BertOutput and
 * `self.dropout` (ref :182).
 * ---------------------------------------------------------------------------------------------- */

/* ------------------------------------------------------------------------------------------------
 * bf16 MFMA GEMM with fused epilogues.  Replaces nn.Linear.forward / its backward inside the HF
 * encoder layers (transformers modeling_bert.py BertSelfAttention.query/key/value,
 * BertSelfOutput.dense, BertIntermediate.dense(+GELU), BertOutput.dense; reached from ref :202-206
 * forward and :841 backward).
 * ---------------------------------------------------------------------------------------------- */
#define CAREL_GEMM_NT 0 /* C[M,N] = A[M,K] * B[N,K]^T          forward: x * W^T                 */
#define CAREL_GEMM_NN 1 /* C[M,N] = A[M,K] * B[K,N]            dgrad:   dY * W                  */
#define CAREL_GEMM_TN 2 /* C[M,N] = A[K,M]^T * B[K,N]          wgrad:   dY^T * X  (split-K)     */

#define CAREL_EPI_BIAS_BF16 0       /* out_bf16 = acc (+ bias)                                   */
#define CAREL_EPI_BIAS_GELU 1       /* out_bf16 = u = acc + bias (optional: NULL skips it) ; out2_bf16 = gelu_erf(u) */
#define CAREL_EPI_BIAS_DROP_RESID 2 /* out_f32 = dropout(acc + bias) + resid_f32                 */
#define CAREL_EPI_DGELU_BF16 3      /* out_bf16 = acc * gelu_erf'(aux_bf16)                      */
#define CAREL_EPI_ADD_F32 4         /* out_f32 = acc (+ resid_f32)                               */
#define CAREL_EPI_SLAB_F32 5        /* out_f32[z] = acc of K-slice z   (z < splits)              */
#define CAREL_EPI_BIAS_GELU_DG 6    /* u = bf16(acc + bias): out_bf16 = gelu_erf'(u) ; out2_bf16 = gelu_erf(u)  (NT form; what the
                                       training encoder saves: the backward epilogue then needs no erf / exp)   */
#define CAREL_EPI_MUL_BF16 7        /* out_bf16 = acc * aux_bf16  (NN form; colsum_part as for DGELU)            */

typedef struct carel_gemm_args {
  const void* A;        /* bf16 */
  const void* B;        /* bf16 */
  int64_t lda, ldb, ldc; /* leading dimensions in elements: lda / ldb multiples of 8; ldc a multiple of 4 for the f32-output epilogues,
                            of 8 for every epilogue with a bf16 output or aux_bf16 (16-byte stores / loads per lane) */
  int32_t M, N, K;      /* NT / NN: N multiple of 96 with K >= 256 (any M; 256 x 96n kernel) or (M,N) multiples of (128,128) / (256,192);
                           TN: (M,N) multiples of (128,128) or (256,192) with K a multiple of 64*splits, or of (256,96) with K a
                           multiple of 64 and at least 4 K tiles of 64 per slice (K / 64 / splits >= 4: the 256 x 96n kernel, which
                           takes such a shape at any grid size and deals the K tiles to the slices as evenly as possible).
                           K is a multiple of 64 in every form */
  int32_t form;         /* CAREL_GEMM_* */
  int32_t epilogue;     /* CAREL_EPI_*  */
  int32_t splits;       /* split-K factor (slab epilogue only), else 1 */
  void* out_bf16;
  void* out2_bf16;
  void* out_f32;        /* slab epilogue: [splits][M][ldc] */
  const void* bias;     /* f32 [N] or NULL */
  const void* resid_f32;
  const void* aux_bf16;
  uint32_t drop_seed, drop_site, drop_idx_offset;
  float drop_p;
  const void* drop_row_map; /* optional int32 [M]: original row of each (packed) row for the dropout element index
                               (= row_map[row] * ldc + col); NULL = identity */
  void* splitk_ws;      /* optional f32 workspace: lets small grids (< 256 tiles, K >= 1536) run split-K into slabs
                           followed by one fused-epilogue pass; results equal up to fp32 summation order */
  int64_t splitk_ws_bytes;
  void* colsum_a;       /* optional, CAREL_GEMM_TN only: f32 [splits][M] = sum over the K (token) dimension of A[k][m] per
                           K-slice, i.e. the bias gradient that goes with the weight gradient; computed with one extra
                           ones-vector MFMA per step in the first tile column */
  void* colsum_part;    /* optional, CAREL_EPI_DGELU_BF16 / CAREL_EPI_MUL_BF16 only: f32 [M/128][N] per-row-tile column sums of the output
                           (pre-rounding); summing them over M/128 gives the FFN1 bias gradient */
  int32_t splitk_ws_zeroed; /* (ABI 5) 1 = the caller zero-filled splitk_ws ONCE when it allocated it and lets nobody else write its last
                           4 KiB: enables pair split-K for N = 768 outputs with K >= 1536 at M ~ 8192 (two workgroups per 256 x 192 tile,
                           each half of K; the second waits for the first's partial sums through per-wave flags kept in that tail, one-
                           directionally, so it cannot deadlock).  0 = never (a stale flag in uninitialised memory could end the wait early). */
  /* ABI 6.  CAREL_EPI_BIAS_DROP_RESID only, all three or none: resid_f32 then holds the PRE-LayerNorm rows h of the LayerNorm whose output
   * is the residual, and the epilogue recomputes LN(h) = (h - mean) * rstd * gamma + beta with the expression of carel_layernorm_fwd
   * (bit-identical to reading its f32 output) -- that LayerNorm call may then pass x_f32 = NULL and not write its 4 B/element at all.
   * resid_ln_stats: f32 [M][2] = mean, rstd as carel_layernorm_fwd stores them; resid_ln_gamma / resid_ln_beta: f32 [ldc]. */
  const void* resid_ln_stats; const void* resid_ln_gamma; const void* resid_ln_beta;
} carel_gemm_args;

int carel_gemm_bf16(const carel_gemm_args* args, void* stream);
/* Split-K factor the library wants for the weight gradient dW[M,N] = dY^T X over T tokens (CAREL_GEMM_TN): pass it as
 * `splits` with an out_f32 of [splits][M][ldc] floats, then carel_slab_reduce_f32.  With the 256 x 96n kernel the T/64
 * K tiles are dealt to the slices as evenly as possible, so T need not be a multiple of 64 * splits. */
int32_t carel_gemm_wgrad_splits(int32_t M, int32_t N, int64_t T);
/* Measurement aid (bench.py roofline leg): while enabled, every carel_gemm_bf16 launch is bracketed by
 * HIP events on its stream.  carel_profile_gemm_read() synchronises and returns the summed kernel time
 * (ms), the summed algorithmic flops (2*M*N*K) and the launch count, then resets the log. */
int carel_profile_gemm(int32_t enable, int32_t max_launches);
int carel_profile_gemm_read(double* total_ms, double* total_flops, int64_t* launches);
/* the two calibration medians of the last read-out, us: an event pair around an empty kernel (what _read subtracts from every
 * bracket), and an event pair with nothing in between */
int carel_profile_gemm_overheads(double* empty_kernel_bracket_us, double* event_pair_us);

/* out[n] (+)= sum_z slabs[z][n];  n multiple of 4 */
int carel_slab_reduce_f32(const void* slabs, void* out, int64_t n, int32_t splits, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Grouped weight gradients (ABI 7): up to four dW_g[M_g, N_g] = dY_g^T X_g over the SAME T tokens -- the four nn.Linear weights of an
 * encoder layer: the dW half of `loss.backward()` (drl_classifier_ec_mmd_final_mul.py:841) for BertSelfAttention q/k/v,
 * BertSelfOutput.dense, BertIntermediate.dense, BertOutput.dense -- in ONE launch of the 256 x 96 ping-pong kernel + one small
 * reduction.  The launch's work list holds whole output tiles (full contraction, written straight into dW: no fp32 slabs) for as
 * many rounds of the 256 CUs as the tile count fills, and splits only the remaining tiles into K slices whose compact partial
 * tiles go through `workspace` and are summed in slice order (bit-reproducible).  An encoder layer at T = 8192: 288 tiles = 256 whole +
 * 32 x 8 slices, 25 MB of workspace traffic instead of the 165 MB of slabs that four split-K launches write and read back.
 * No workgroup waits for another one.  db (optional) = column sums of dY = the bias gradient of the same linear, from ones-vector MFMAs
 * in the first tile column.  ln[] (optional): the per-block partials of up to two LayerNorm backward passes (carel_layernorm_bwd's scratch
 * layout), summed into dgamma / dbeta / dbias by the same reduction launch (the arithmetic of carel_layernorm_bwd's own second pass).
 * M_g multiple of 256 (<= 4096), N_g multiple of 96 (<= 3072), T multiple of 64 (>= 256); every pointer 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_wgrad_problem {
  const void* dY;   /* bf16 [T, M] row-major */
  const void* X;    /* bf16 [T, N] row-major */
  void* dW;         /* f32 [M, N] (nn.Linear weight layout) */
  void* db;         /* f32 [M] or NULL */
  int32_t M, N;
} carel_wgrad_problem;
typedef struct carel_ln_partial_set {
  const void* partials;   /* f32 [carel_layernorm_bwd_blocks(rows)][3 * 768] */
  int64_t rows;
  void* dgamma; void* dbeta; void* dbias;   /* f32 [768] each; any may be NULL */
} carel_ln_partial_set;
typedef struct carel_wgrad_group_args {
  carel_wgrad_problem prob[4];
  int32_t n_prob;         /* 1..4 */
  int64_t T;
  void* workspace;        /* carel_gemm_wgrad_group_ws_bytes(args) bytes (may be 0: every tile whole) */
  int64_t workspace_bytes;
  carel_ln_partial_set ln[2];
  int32_t n_ln;           /* 0..2 */
} carel_wgrad_group_args;
/* workspace size for these shapes (pointers are not read); -1 if the shapes cannot run grouped */
int64_t carel_gemm_wgrad_group_ws_bytes(const carel_wgrad_group_args* args);
int carel_gemm_wgrad_group(const carel_wgrad_group_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Embeddings + LayerNorm (HF BertEmbeddings / RobertaEmbeddings.forward) and its backward.
 *   x0 = dropout(LN(word[ids] + pos[position_ids] + type[token_type_ids])), dropout site 0.
 * position_ids: arange(S) for BERT; cumsum(ids != pad) * (ids != pad) + pad for RoBERTa (roberta = 1).
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_embed_args {
  const void* input_ids;       /* int64 [B, S] */
  const void* token_type_ids;  /* int64 [B, S] or NULL (= 0) */
  const void* word_emb;        /* f32 [vocab, 768]   */
  const void* pos_emb;         /* f32 [max_pos, 768] */
  const void* type_emb;        /* f32 [type_vocab, 768] */
  const void* ln_gamma;        /* f32 [768] */
  const void* ln_beta;         /* f32 [768] */
  float ln_eps;
  int32_t batch, seq_len, hidden;        /* hidden must be 768 */
  int32_t vocab_size, max_pos, type_vocab; /* type_vocab 1 or 2 */
  int32_t roberta, pad_id;
  uint32_t drop_seed, drop_idx_offset;
  float drop_p;
  void* x_f32;                 /* out f32  [B*S, 768] */
  void* x_bf16;                /* out bf16 [B*S, 768] */
  void* stats;                 /* out f32  [B*S, 2] (mean, rstd); input of the backward */
  /* token packing (padding skipped): row t of the outputs is original row tok_row[t] (= b*S + s), -1 = filler
   * row (written as zeros); n_rows rows are produced.  NULL / 0 = dense (row t = original row t, B*S rows). */
  const void* tok_row;         /* int32 [n_rows] or NULL */
  int32_t n_rows;
} carel_embed_args;

int carel_embed_ln_fwd(const carel_embed_args* args, void* stream);
/* number of row blocks of the backward kernels: partial buffers need blocks * slots * 768 floats */
int carel_embed_ln_bwd_blocks(int64_t rows);
/* dword [vocab,768] and dpos [max_pos,768] are ACCUMULATED into with float atomics (zero them first);
 * dtype [type_vocab,768], dgamma, dbeta [768] are overwritten.
 * partials: f32 scratch, carel_embed_ln_bwd_blocks(B*S) * (2 + type_vocab) * 768 floats. */
int carel_embed_ln_bwd(const carel_embed_args* args, const void* dx0_f32, void* dword, void* dpos, void* dtype,
                       void* dgamma, void* dbeta, void* partials, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm over 768-wide rows (BertSelfOutput.LayerNorm / BertOutput.LayerNorm) and its backward with
 * the sub-layer dropout backward fused:  dh = LN'(dy) ; dy_bf16 = dh * dropout_mask(site) ;
 * dgamma, dbeta, dbias (= column sum of dy_bf16 before rounding) are overwritten.
 * ---------------------------------------------------------------------------------------------- */
int carel_layernorm_fwd(const void* h_f32, const void* gamma, const void* beta, float eps, int64_t rows, int32_t hidden,
                        void* x_f32, void* x_bf16, void* stats, void* stream);
/* number of partial blocks the backward kernel writes for EXACTLY this row count (4, 8 or 16 rows per block: fewer rows per block at small
 * row counts, so the value is NOT monotonic in `rows` -- 2048 rows: 512 blocks, 2064 rows: 258; size a buffer that is reused for several row
 * counts with the largest value over them; never more than max(512, ceil(rows / 16)) for any smaller count) */
int carel_layernorm_bwd_blocks(int64_t rows);
/* partials: f32 scratch of carel_layernorm_bwd_blocks(rows) * 3 * 768 floats */
int carel_layernorm_bwd(const void* dy_f32, const void* h_f32, const void* stats, const void* gamma, int64_t rows,
                        int32_t hidden, uint32_t drop_seed, uint32_t drop_site, uint32_t drop_idx_offset, float drop_p,
                        void* dh_f32, void* dy_bf16, void* dgamma, void* dbeta, void* dbias, void* partials, void* stream);
/* same with packed rows: drop_row_map int32 [rows] gives each row's original row for the dropout index */
int carel_layernorm_bwd_packed(const void* dy_f32, const void* h_f32, const void* stats, const void* gamma, int64_t rows,
                               int32_t hidden, uint32_t drop_seed, uint32_t drop_site, uint32_t drop_idx_offset, float drop_p,
                               const void* drop_row_map, void* dh_f32, void* dy_bf16, void* dgamma, void* dbeta, void* dbias,
                               void* partials, void* stream);
/* out[c] (+)= sum_p partials[p][c]  (c < n, p < nparts), fixed summation order */
int carel_partial_reduce_f32(const void* partials, void* out, int32_t n, int32_t nparts, int32_t accumulate, void* stream);
/* out[n] (+)= column sums of a bf16 matrix [rows, n] (bias gradients); partials: ceil(rows/256)*n floats */
int carel_colsum_bf16(const void* x_bf16, int64_t ld, int64_t rows, int32_t n, void* out_f32, int32_t accumulate,
                      void* partials, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Self-attention of one encoder layer, all (sample, head) pairs; S a multiple of 32 in [32, 512], 12 heads x 64.
 * S <= 128: one workgroup per (sample, head), all of K and V in LDS (attention.hip).  S > 128 (ABI 9): flash-style kernels
 * (attention_long.hip): the forward walks 128-key blocks with an online softmax; the backward runs a dQ pass over 128-query blocks
 * and a dK / dV pass over 128-key blocks (no atomics: every gradient bit-reproducible) and needs `workspace`.  With dropout on,
 * drop_idx_offset must be even (the kernels hash whole pairs of elements) and batch * 12 * S * S + drop_idx_offset must not exceed 2^32
 * (the element index is 32-bit; S = 512: about 1 365 samples per call); both are refused with an error before any launch.
 * A sample with no attended key (all-zero mask) gets HF's uniform row in the forward, but exact zeros in all of its dQ / dK / dV rows
 * in the backward, where HF autograd would give nonzero dK / dV (no input of the encoder has such a sample).
 * Replaces transformers BertSelfAttention.forward after the q/k/v projections (eager attention:
 * softmax(QK^T/8 + (1-mask)*finfo.min) -> dropout -> PV) and its backward.
 * qkv / dqkv: bf16 [B*S, 2304] = q | k | v.  ctx / dctx: bf16 [B*S, 768].  lse: f32 [B, 12, S].
 * dropout element index = ((b*12 + h)*S + q)*S + k.
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_attn_args {
  const void* qkv;
  const void* attention_mask;  /* int64 [B, S], 1 = attend; NULL = all ones */
  void* ctx;                   /* fwd: out; bwd: in */
  void* lse;                   /* fwd: out; bwd: in */
  const void* dctx;            /* bwd in  */
  void* dqkv;                  /* bwd out */
  int32_t batch, seq_len, heads, head_dim;
  uint32_t drop_seed, drop_site, drop_idx_offset;   /* drop_idx_offset: even when drop_p > 0 */
  float drop_p;
  /* token packing: sample b owns rows [cu_seqlens[b], cu_seqlens[b+1]) of qkv/ctx/dctx/dqkv and attends to exactly
   * those (attention_mask is ignored); seq_len stays the ORIGINAL padded length (dropout index, lse stride). */
  const void* cu_seqlens;      /* int32 [B+1] or NULL */
  /* MPNet relative-position bias (transformers MPNetAttention: attention_scores += position_bias; the encoder of
   * en_ec_sentence_transformer.py:22): f32 [heads][256], entry 127 + (key position - query position), made from the learned
   * [32 buckets][heads] table by carel_relpos_expand; NULL = no bias (BERT / RoBERTa). */
  const void* rel_bias_dist;   /* S > 128: f32 [heads][1024], entry 511 + (key - query) (entry 1023 unused), by carel_relpos_expand_span */
  void* d_rel_bias_dist;       /* bwd, required with rel_bias_dist: f32 [batch * heads][256] (S > 128: [batch * heads][1024], entry as above), row (sample, head) ADDED to by that workgroup alone
                                  (no atomics: bit-reproducible); the caller zeroes it once per step -- every layer adds to it -- and folds
                                  it into the table gradient with carel_relpos_reduce */
  int32_t q_rows;              /* ABI 6.  0 = every query row; 32 / 64 / 96: only the first q_rows positions of every sample are queries --
                                  forward: ctx / lse rows past them are NOT written; backward: dctx rows past them are taken as zero and
                                  their dQ rows are written as zeros.  Exact where nothing downstream reads the other rows: the encoder's
                                  last layer when only [CLS] (position 0) is read after it (carel_encoder_args.n_cls) */
  /* ABI 9.  bwd with S > 128: carel_attention_bwd_workspace_bytes(batch, seq_len, rel_bias_dist != NULL) bytes of device memory
   * (f32 delta = rowsum(dO * O) [batch * heads * S], then with the bias its gradient partials [batch * heads][S/128 rounded up][1024]);
   * contents need not be kept between calls.  Unused (may be NULL / 0) for S <= 128 and in the forward. */
  void* workspace;
  int64_t workspace_bytes;
} carel_attn_args;

int carel_attention_fwd(const carel_attn_args* args, void* stream);
int carel_attention_bwd(const carel_attn_args* args, void* stream);
/* bucket: int32 [256], bucket[i] = relative_position_bucket(i - 127) (entry 255 unused), computed by the caller */
/* (both are the span-256 calls of carel_relpos_expand_span / carel_relpos_reduce_span below) */
int carel_relpos_expand(const void* table_f32_32xH, const void* bucket, void* dist_f32_Hx256, void* stream);
int carel_relpos_reduce(const void* ddist_f32_BHx256, int32_t batch, const void* bucket, void* dtable_f32_32xH, int32_t accumulate, void* stream);
/* ABI 9: 0 for seq_len <= 128 */
int64_t carel_attention_bwd_workspace_bytes(int32_t batch, int32_t seq_len, int32_t with_rel);
/* ABI 9: the same for a span of 256 (S <= 128; the bits of the two calls above) or 1024 (S > 128): bucket int32 [span],
 * bucket[i] = relative_position_bucket(i - (span/2 - 1)) (entry span - 1 unused); dist f32 [H][span]; ddist f32 [batch * H][span] */
int carel_relpos_expand_span(const void* table_f32_32xH, const void* bucket, void* dist_f32_Hxspan, int32_t span, void* stream);
int carel_relpos_reduce_span(const void* ddist_f32_BHxspan, int32_t batch, const void* bucket, void* dtable_f32_32xH, int32_t accumulate,
                             int32_t span, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-encoder orchestration over caller-owned buffers.  Replaces `self.encoder(...)` (ref :202-206;
 * transformers BertModel / RobertaModel forward) and the encoder part of `loss.backward()` (ref :841).
 * Weights are read as bf16 (the shadow copy maintained by carel_adam_step / carel_cast_f32_to_bf16),
 * biases / LayerNorm parameters / embeddings as f32.  The q/k/v projections are one fused [2304,768]
 * matrix (query rows, then key, then value).
 *   act     : carel_encoder_act_bytes(B, S, L, inference) bytes; holds every activation the backward
 *             needs (inference = 1: one layer's worth, re-used by every layer; no backward possible)
 *   scratch : carel_encoder_scratch_bytes(B, S) bytes of workspace.  ZERO-FILL IT ONCE when it is allocated, and let nothing but the library
 *             write to it afterwards (ABI 5): a few words of it are flags of the pair split-K GEMMs (carel_gemm_args.splitk_ws_zeroed), which
 *             must not start out equal to a launch sequence number.  A training forward (inference = 0, scratch != NULL,
 *             B*S or n_tokens <= 8192 rows, vocab_size and max_pos < 2^19) also leaves the batch's sorted embedding keys in it;
 *             carel_encoder_backward_embeddings then writes the word / position table gradients as fixed-order sums
 *             (bit-reproducible) if the last forward that wrote keys into this scratch had the same act, input_ids, tok_row and
 *             row count and no later forward ran on that act.  Otherwise (a forward with scratch = NULL or with other ids, any
 *             forward in between on the same act) it falls back to float atomics: correct, not bit-reproducible.  The record is kept
 *             on the host by pointer: rewriting input_ids in place between forward and backward breaks the pairing unnoticed.
 *             seq_len > 128 (ABI 9): the scratch also holds the long-sequence attention backward's workspace
 *             (carel_attention_bwd_workspace_bytes with the bias partials); a dense long batch passes 8 192 rows from B*S = 8 320 on
 *             (e.g. B = 17 at S = 512), and its embedding gradients then take the atomic path above
 *   dx      : f32 [B*S, 768]; in: d(loss)/d(last hidden state); carried down through the layers
 * Constraints: hidden 768, 12 heads, intermediate 3072, seq_len a multiple of 32 in [32, 512] (ABI 9; 160 .. 512 run the flash-style
 * attention kernels, 32 .. 128 the one-workgroup-per-(sample, head) ones), B*S % 128 == 0; carel_embed_ln_fwd (the embeddings) also
 * needs seq_len <= max_pos (BERT) or <= max_pos - pad_id - 1 (RoBERTa / MPNet: position ids from pad_id + 1).  carel_encoder_forward_f32
 * stays at seq_len <= 128.
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_layer_params {
  const void* qkv_w; const void* qkv_b;     /* bf16 [2304,768], f32 [2304] */
  const void* out_w; const void* out_b;     /* bf16 [768,768],  f32 [768]  */
  const void* ln1_g; const void* ln1_b;     /* f32 [768] */
  const void* ffn1_w; const void* ffn1_b;   /* bf16 [3072,768], f32 [3072] */
  const void* ffn2_w; const void* ffn2_b;   /* bf16 [768,3072], f32 [768]  */
  const void* ln2_g; const void* ln2_b;     /* f32 [768] */
} carel_layer_params;

typedef struct carel_layer_grads {          /* all f32, shapes as above */
  void* qkv_w; void* qkv_b; void* out_w; void* out_b; void* ln1_g; void* ln1_b;
  void* ffn1_w; void* ffn1_b; void* ffn2_w; void* ffn2_b; void* ln2_g; void* ln2_b;
} carel_layer_grads;

typedef struct carel_encoder_args {
  int32_t batch, seq_len, n_layers, hidden, heads, intermediate;
  int32_t vocab_size, max_pos, type_vocab, roberta, pad_id, inference;
  float ln_eps, hidden_dropout, attn_dropout;
  uint32_t drop_seed, drop_row_offset;      /* row offset = global index of this shard's first sample */
  const void* input_ids; const void* attention_mask; const void* token_type_ids;   /* int64 [B,S] */
  const void* word_emb; const void* pos_emb; const void* type_emb; const void* emb_ln_g; const void* emb_ln_b; /* f32 */
  const carel_layer_params* layers;         /* HOST array [n_layers] of device pointers */
  void* act; void* scratch;
  /* token packing (skip padded positions; results identical for prefix-form attention masks):
   * n_tokens = packed row count rounded up to 128, tok_row int32 [n_tokens] (original row or -1),
   * cu_seqlens int32 [B+1].  n_tokens = 0 / NULL pointers = dense. */
  int32_t n_tokens; const void* tok_row; const void* cu_seqlens;
  /* dead-row elimination: nothing but the [CLS] row of the last layer's output is ever read (HF BertPooler), so the last
   * layer runs its row-wise part (out-proj, LayerNorm, FFN, LayerNorm) and their backward on the n_cls (= batch rounded
   * up to 128) [CLS] rows only; results are unchanged.  cls_rows int32 [n_cls]: row of sample i's [CLS] token in the
   * current (dense or packed) row space, -1 for filler; cls_orig_rows int32 [n_cls]: its original row i*S (dropout
   * index), -1 for filler.  The final hidden states (carel_encoder_x_last) are then the n_cls compact rows, and dx is
   * read as n_cls compact rows by the backward of the last layer.  n_cls = 0 disables. */
  int32_t n_cls; const void* cls_rows; const void* cls_orig_rows;
  /* bit 0 (1): carel_encoder_backward_layer enqueues the weight-gradient GEMMs (and their slab / bias-gradient reductions) on a
   * library-owned low-priority second stream, forked by events behind the kernel that produced each dY, so that they
   * run beside the data-gradient chain and the memory-bound LayerNorm / attention backward kernels; bit 1 (2): the
   * forward pass runs the two halves of a dense batch as two chains (second chain on a peer stream).  3 = both.
   * Results are identical (same kernels, same summation order).
   * COMPLETION: in the order of `stream`, after carel_encoder_backward_layer(l) returns the parameter gradients of
   * layer l+1 are complete; those of layer l after the next call, carel_encoder_backward_join or
   * carel_encoder_backward_embeddings.  0: everything on `stream`, every layer complete when its call returns. */
  int32_t overlap_wgrad;
  const carel_layer_grads* layer_grads;     /* HOST array [n_layers] */
  void* d_word_emb; void* d_pos_emb; void* d_type_emb; void* d_emb_ln_g; void* d_emb_ln_b;
  void* dx;
  /* MPNet relative-position bias, shared by all layers (see carel_attn_args): NULL = none.  d_rel_bias_dist is accumulated into by
   * every layer's attention backward; the caller zeroes it before the first carel_encoder_backward_layer of a step. */
  const void* rel_bias_dist; void* d_rel_bias_dist;
} carel_encoder_args;

/* The library's two low-priority streams of the current device (created on first use, never destroyed):
 * 0 = the weight-gradient stream used by overlap_wgrad, 1 = an auxiliary stream the host side uses for work that may
 * trail the backward pass (the per-layer Adam updates of FusedAdam(fuse_into_backward=True)).  NULL on failure. */
void* carel_side_stream(int32_t which);
int carel_encoder_backward_join(const carel_encoder_args* args, void* stream);
int64_t carel_encoder_act_bytes(int32_t batch, int32_t seq_len, int32_t n_layers, int32_t inference);
int64_t carel_encoder_scratch_bytes(int32_t batch, int32_t seq_len);
/* device pointer (inside act) of the final hidden states, f32 [B*S, 768] */
void* carel_encoder_x_last(const carel_encoder_args* args);
int carel_encoder_forward(const carel_encoder_args* args, void* stream);
/* fp32 DEBUG forward (forward only, dropout off, dense batches): the same graph with every stored value in fp32 -- linears on the
 * f32-input matrix cores (carel_sgemm_f32), attention, GELU and LayerNorm in fp32 -- so that a difference from the fp32 reference
 * (BertModel.forward, drl_classifier_ec_mmd_final_mul.py:202-206) is kernel error, not bf16 rounding (tests assert <= 1e-5 against
 * the reference's own fp32 outputs).  Here args->layers[i].*_w point to F32 weights (same shapes); args->act / scratch / n_cls are
 * not used.  work: carel_encoder_f32_work_bytes(batch, seq_len) bytes; x_out: f32 [batch*seq_len, 768] final hidden states.
 * seq_len <= 128.  ~20x slower than carel_encoder_forward: a measurement tool, not a product path. */
int64_t carel_encoder_f32_work_bytes(int32_t batch, int32_t seq_len);
int carel_encoder_forward_f32(const carel_encoder_args* args, void* work, void* x_out_f32, void* stream);
/* One layer of the backward pass.  Call for layer = n_layers-1 down to 0 after a training forward: a pass STARTS with the last layer
 * (with token packing that call also clears the filler rows of the shared dqkv scratch, which the later calls of the pass rely on). */
int carel_encoder_backward_layer(const carel_encoder_args* args, int32_t layer, void* stream);
int carel_encoder_backward_embeddings(const carel_encoder_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * VAE tail of DrlClassifier.forward (ref :202-261): pooler -> latent heads -> sample -> emotion CE,
 * cause BCE, pair BCE-with-logits(pos_weight), RBF-MMD, annealed KL, decoder softmax + BCE; and the
 * backward of all of it.  fp32 throughout.
 *
 *   carel_tail_latents : pooled = tanh(W_p x_last[:,0] + b_p) (HF BertPooler); lat = [mu_e|lv_e|mu_c|lv_c]
 *                        (ref :312-336).  Also the front half of get_pair_preds (ref :266-275).
 *   carel_tail_losses  : z, terms[0..8] and d(loss)/d(parameter) for the classifier heads + decoder,
 *                        d(loss)/d lat kept in `work`.   terms = {partial, mmd, emo, cau, pair, kl_e,
 *                        kl_c, rec, loss}; loss = w_mmd*(-mmd) + w_emo*emo + w_cau*cau + w_pair*pair +
 *                        kl_e + kl_c + rec (ref :256-261); kl_* already multiplied by kl_weight.
 *   carel_tail_backward: latent heads + pooler backward -> d_head_*, d_pooler_*, dx_last (zero except
 *                        the CLS rows), all scaled by *grad_out_dev (NULL = 1).
 *   carel_pair_probs   : sigmoid(pair_classifier([mu_e + eps_e e^lv_e, mu_c + eps_c e^lv_c])) (ref :277-282)
 * Data-parallel hooks (all optional): global_label_sum/global_n give the pos_weight of the GLOBAL batch;
 * z_global [global_n, 2*ec_dim] (all-gathered samples) + global_row_offset make the MMD the global-batch
 * statistic, differentiated for the local rows and scaled by mmd_grad_scale (= world size when gradients
 * are averaged over ranks).
 * Batch limit of carel_tail_losses: its loss kernel (one workgroup) and its decoder kernels keep the whole batch in the 160 KB
 * LDS of one CU, so the largest batch depends on ec_dim (and, by one sample at most, on e_classes).  At 6 emotion classes:
 *     ec_dim | decoder accepts B <= | loss kernel accepts B <=
 *        8   |        142           |        363
 *       16   |        127           |        211
 *       24   |        114           |        149
 *       32   |        101           |        115
 * The smaller figure holds (any bow_dim).  A larger batch (and batch < 2 without z_global) returns CAREL_ERR_SHAPE before
 * anything is launched: no output is touched and no work is left on the side stream.  The table belongs to carel_tail_losses
 * alone; carel_tail_batch_limit(ec_dim, e_classes) computes it from the same two LDS plans.
 *
 *   carel_tail_losses_tiled : the batch-tiled form of carel_tail_losses for batches beyond that limit.  Same contract (needs
 *                        carel_tail_latents first), same outputs (z, terms[0..8], the six classifier gradients, the decoder
 *                        gradients, the pair_dead flag, d(loss)/d lat in `work` for carel_tail_backward[_dz]), same workspace,
 *                        same dropout streams from the same element indices, same data-parallel hooks.  The heads / losses / KL
 *                        run over slabs of 64 rows in two phases (the pair label sum, the divisor of every mean and the "dead"
 *                        decision on the batch-mean pair loss are those of the whole batch), the MMD in the row-blocked kernel
 *                        of the global-batch path, the decoder passes over tiles of 32 (ec_dim <= 25) or 16 rows; LDS per
 *                        workgroup is below 64 KB whatever the batch.  No atomics: every sum has an order fixed by indices, a
 *                        repeated call gives the same bits (which differ from carel_tail_losses' in the last places, the sums
 *                        being ordered differently; z is bit-identical).
 *                        Limits: 2 <= batch <= 1024 (1 with z_global; small batches are accepted), ec_dim <= 32, e_classes <= 8,
 *                        both emotion heads, dis_mode 0 (MMD) and 2 (none).  dis_mode 1 (HSIC) keeps the single-workgroup
 *                        limit: CAREL_ERR_SHAPE, the message names the limit.  Every check comes before the first launch: a
 *                        refused call touches no output and leaves nothing enqueued.  Everything runs on `stream` (`serial` is
 *                        ignored, the side stream is not used), so the call is re-entrant.
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_tail_args {
  int32_t batch, seq_len, hidden, ec_dim, e_classes, bow_dim;
  const void* x_last_f32;            /* f32 [B*S, 768] last encoder LayerNorm output */
  const void* pooler_w; const void* pooler_b;
  const void* head_w[4]; const void* head_b[4];   /* emotion_mu, emotion_log_var, cause_mu, cause_log_var */
  const void* emo_w; const void* emo_b;
  const void* cau_w; const void* cau_b;
  const void* pair_w; const void* pair_b;
  const void* dec_w; const void* dec_b;
  const void* emo_labels;            /* int64 [B] */
  const void* cau_labels;            /* f32 [B] */
  const void* pair_labels;           /* f32 [B] */
  const void* bow;                   /* f32 [B, bow_dim] */
  const void* eps_e; const void* eps_c; /* f32 [ec_dim] */
  float w_mmd, w_emo, w_cau, w_pair, kl_weight, label_smoothing;
  float drop_p; uint32_t drop_seed, drop_row_offset;
  float mmd_alpha, mmd_eps;
  int32_t dis_mode;                  /* disentanglement term: 0 = -w_mmd * RBF-MMD (ref :231-233, :256);
                                        1 = +w_mmd * HSIC(z_e, z_c) (drl_classifier_ec_hsic.py:214, :253; w_mmd = 1 there); 2 = none */
  int32_t emo_bce;                   /* 1 = one-logit sigmoid + BCE emotion head of the ablation scripts
                                        (drl_classifier_ec_hsic.py:455-470; e_classes must be 1, labels 0/1), 0 = softmax CE (ref :461-476) */
  const void* global_label_sum;      /* f32 [1] or NULL */
  int32_t global_n, global_row_offset;
  const void* z_global;              /* f32 [global_n, 2*ec_dim] or NULL */
  float mmd_grad_scale;
  int32_t global_rank_stride;        /* 0: z_global is dense; else floats between the blocks of `batch` rows contributed by
                                        consecutive ranks (lets one all-gather carry z plus a few extra floats per rank) */
  int32_t global_label_ranks;        /* > 1: the global label sum is the sum of this many floats starting at
                                        global_label_sum, global_rank_stride apart (each rank's own sum, straight out of
                                        the same all-gather); 0 / 1: global_label_sum[0] is already the total */
  /* outputs */
  void* pooled;                      /* f32 [B, 768] */
  void* lat;                         /* f32 [B, 4*ec_dim] */
  void* z;                           /* f32 [B, 2*ec_dim] */
  void* terms;                       /* f32 [16] */
  void* work;                        /* f32 [carel_tail_workspace_floats(...)] */
  void* d_emo_w; void* d_emo_b; void* d_cau_w; void* d_cau_b; void* d_pair_w; void* d_pair_b;
  void* d_dec_w; void* d_dec_b;
  void* d_head_w[4]; void* d_head_b[4];   /* may be NULL (heads are not optimised, ref :292-295) */
  void* d_pooler_w; void* d_pooler_b;
  void* dx_last_f32;                 /* f32 [B*S, 768] (packed: [n_rows, 768]) */
  const void* cls_rows;              /* int32 [B]: row of each sample's [CLS] token in x_last / dx_last; NULL = b*seq_len */
  int32_t n_rows;                    /* rows of dx_last to clear (0 = B*seq_len) */
  int32_t serial;                    /* ABI 6.  0: carel_tail_losses may run its single-workgroup loss kernel on the library's side stream
                                        (carel_side_stream(0)) beside the decoder passes on `stream`, forked and joined with events inside
                                        the call -- `stream` order is all a caller ever sees; 1: every kernel on `stream`, in order
                                        (serial kernel traces, per-launch timing) */
  /* ABI 8: the sentence adapters of drl_classifier_ec_mmd_final_mul_emnlp.py (:334-354; carel_adapter_* below).  NULL (default):
   * the pooler path above, unchanged.  Set: the latent heads read these rows instead of the pooler --
   *   head_in_f32   f32 [2, B, 768]: block 0 = emotion adapter output (read by emotion_mu / emotion_log_var),
   *                 block 1 = cause adapter output (cause_mu / cause_log_var); carel_tail_latents skips the pooler (`pooled` unwritten);
   *   d_head_in_f32 f32 [2, B, 768]: carel_tail_backward writes d loss / d head_in here (scaled by grad_out) instead of running the
   *                 pooler backward and the [CLS] scatter; dx_last_f32 is left to carel_adapter_backward, and d_pooler_w / d_pooler_b
   *                 (when given) are zero-filled -- the pooler is unused (its gradient is None in the reference). */
  const void* head_in_f32;
  void* d_head_in_f32;
} carel_tail_args;

int64_t carel_tail_workspace_floats(int32_t batch, int32_t ec_dim, int32_t bow_dim);
/* pooled, lat and -- when eps_e / eps_c / z are given -- the sampled embeddings z (so that a data-parallel caller can
 * all-gather z before carel_tail_losses, which recomputes the same z) */
int carel_tail_latents(const carel_tail_args* args, void* stream);
int carel_tail_losses(const carel_tail_args* args, void* stream);
/* HOST function: the largest batch carel_tail_losses accepts at this width (without z_global), 0 for widths the tail refuses */
int32_t carel_tail_batch_limit(int32_t ec_dim, int32_t e_classes);
int carel_tail_losses_tiled(const carel_tail_args* args, void* stream);
/* Measurement aid: while a device buffer of 16 int64 is registered, the fused loss kernel of carel_tail_losses writes
 * 100 MHz time stamps at its phase boundaries into it (NULL switches it off). */
int carel_tail_profile(void* dev_i64_x16);
int carel_tail_backward(const carel_tail_args* args, const void* grad_out_dev_f32, void* stream);
/* same, plus an additional upstream gradient on the sampled embeddings z (f32 [B, 2*ec_dim], NOT scaled by grad_out):
 * lets further loss terms defined on z_e / z_c (e.g. the CLUB bound of the VI ablation) reach the encoder */
int carel_tail_backward_dz(const carel_tail_args* args, const void* grad_out_dev_f32, const void* dz_extra_f32, void* stream);
/* Host->device feeding of the bag-of-words targets (`bow_reps.to(device)`, ref :829, 6 MB per batch when dense): the batch's
 * non-zeros as triples -- trip = int32 rows[nnz], int32 cols[nnz], f32 vals[nnz], contiguous, distinct (row, col) -- are
 * expanded into the dense f32 [B, V] block the loss kernels read (zero fill + scatter, stream-ordered). */
int carel_bow_expand(const void* trip, int32_t nnz, void* out_f32, int32_t B, int32_t V, void* stream);
/* HOST function (no HIP call, no GIL when reached through ctypes): gather the dataset rows idx[0..batch) into one staging
 * block of 4-byte words -- the seven tensors of a batch (ref :136-144, :823-830) back to back at the given word offsets
 * (int64 fields 8-byte aligned), the bag-of-words targets as rows[B*M], cols[B*M] (-1 = padding), vals[B*M] at off_trip.
 * Every source pointer is a HOST array stacked over the n_samples of the dataset. */
typedef struct carel_host_pack_args {
  const void* input_ids; const void* attention_masks; const void* token_type_ids;   /* int64 [n, S] */
  const void* labels; const void* cau_labels;                                     /* f32 [n] */
  const void* emo_labels;                                                         /* int64 [n] or f32 [n] (emo_is_float) */
  const void* bow_cols; const void* bow_vals;                                     /* int32 / f32 [n, M] */
  const int64_t* idx;                                                             /* [batch] sample indices */
  void* dst;                                                                      /* staging block (page-locked) */
  int64_t n_samples;
  int32_t batch, seq_len, bow_entries, emo_is_float;
  int64_t off_input_ids, off_attention_masks, off_token_type_ids, off_labels, off_cau_labels, off_emo_labels, off_trip;
  /* optional token packing (padding skipped, carel_encoder_args.tok_row / cu_seqlens): lengths = int32 [n] attended
   * length of every sample; writes cu_seqlens int32 [batch_padded + 1] at off_cu and tok_row int32 [<= batch*seq_len rounded up to 128] at
   * off_tok, returns the attended-token count and its round-up to 128 in t_eff / t_pad.  lengths = NULL: skipped. */
  const void* lengths;
  int32_t batch_padded;
  int64_t off_cu, off_tok;
  int64_t t_eff, t_pad;                                                           /* out */
} carel_host_pack_args;
int carel_host_pack_batch(carel_host_pack_args* args);
/* x[i] *= *scale_dev  (device scalar: no host sync).  A utility for callers of the C ABI that scale the classifier / decoder gradients
 * of carel_tail_losses in place; the Python models add grad_output x those gradients into .grad with carel_axpy_f32 instead. */
int carel_scale_f32(void* x_f32, int64_t n, const void* scale_dev_f32, void* stream);
/* offset (in floats, inside `work`) of the flag carel_tail_losses sets to 1.0 when the pair loss was
 * replaced by 0 (ref :510-511); carel_adam_step's skip_flag points at it */
int64_t carel_tail_pair_dead_offset(int32_t batch, int32_t ec_dim, int32_t bow_dim);
int carel_pair_probs(const void* lat, const void* eps_e, const void* eps_c, const void* pair_w, const void* pair_b,
                     int32_t batch, int32_t ec_dim, void* prob, void* stream);
/* carel_pair_probs for n_draws noise vectors over the same latents (the case analysis re-evaluates the test set with fresh noise until
 * its F1 crosses a threshold, mmd_wommd_case_analysis.py:662-696; in eval mode only eps changes between draws).
 *   lat [n, 4*ec_dim] f32, eps_e / eps_c [n_draws, ec_dim] f32, pair_w [2*ec_dim], pair_b [1]
 *   prob    f32 [n_draws, n] or NULL; every entry has the bits carel_pair_probs gives for that draw's eps
 *   labels  f32 [n] (positive: == 1) or NULL; groups int32 [n] in [0, n_groups) or NULL (all rows in group 0); n_groups in 1..8
 *   counts  int32 [n_draws, n_groups, 3] = TP, FP, FN with the prediction prob > 0.5, or NULL; needs labels; written in full by the
 *           call (no pre-zeroing); a row whose group id is outside [0, n_groups) is counted nowhere
 * At least one of prob / counts; ec_dim in 1..32; n, n_draws >= 1.  Integer counting only: the same bits on every launch. */
int carel_pair_probs_draws(const void* lat, const void* eps_e, const void* eps_c, const void* pair_w, const void* pair_b,
                           int32_t n, int32_t ec_dim, int32_t n_draws, void* prob, const void* labels, const void* groups,
                           int32_t n_groups, void* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sentence adapters (ABI 8) of drl_classifier_ec_mmd_final_mul_emnlp.py / ..._newsplit_emnlp.py: the emotion and the cause latent
 * branches each read their own attention adapter over EVERY position of the last hidden state H [B, S, 768] (:334-354, get_pair_preds
 * :420-442) instead of the pooler.  A fixed query e (emotion_q / cause_q, :275 / :284) attends over all S positions; no mask, so
 * padded positions are attended too.
 *   mode 1 sparsemax (SparsemaxMultiheadAttention, :162-210), mode 2 entmax15 (EntmaxMultiheadAttention, :213-256), G = 1:
 *       scores[b,s] = q_proj(e) . k_proj(H[b,s]) / sqrt(768);  p = normaliser(scores[b,:]);  out[b] = sum_s p[b,s] H[b,s]
 *       (value = the raw H; v_proj, in_proj_* and out_proj exist but are unused there);
 *   mode 0 raw (nn.MultiheadAttention(768, G, batch_first=True) called as (e, H, H), :277 / :286), G = head_number:
 *       per head h: softmax(q_h . k_h(H) / sqrt(768/G)), v = in_proj_v(H), then out_proj.
 * Every normaliser is translation-invariant, so the key bias drops out and the key projection reassociates exactly:
 *   u_h = W_k,h^T q_h / sqrt(d)  (carel_adapter_build_u),  scores_h[b,s] = H[b,s] . u_h
 * -- no [B*S, 768] x [768, 768] GEMM.  For raw mode the value projection and out_proj act after the weighted sum (sum_s p = 1).
 * Both adapters go through one pass over H.  f32 throughout; exact sort-based normalisers (ties included); no atomics (results
 * are bitwise repeatable).  seq_len in {32, 64, 96, 128}; G | 768, G <= 12; G = 1 for modes 1 / 2; batch_padded <= 65535;
 * u, work, x, out, d_out, dx, query and the weight matrices 16-byte aligned (anything else is refused before any launch).
 *
 * Weights per adapter a (0 = emotion, 1 = cause), each [768, 768] row-major (nn.Linear layout) / [768]:
 *   modes 1 / 2: q_w / q_b = q_proj, k_w = k_proj.weight;   v_* / o_* unused (may be NULL)
 *   mode 0:      q_w / q_b = in_proj rows 0..767, k_w = in_proj rows 768..1535, v_w / v_b = in_proj rows 1536..2303, o_w / o_b = out_proj
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_adapter_args {
  int32_t batch;                     /* B real samples */
  int32_t batch_padded;              /* Bp >= B: samples (of seq_len rows each) in x / dx; the filler samples' dx rows are written 0 */
  int32_t seq_len;                   /* S */
  int32_t mode;                      /* 0 raw (softmax), 1 sparsemax, 2 entmax15 */
  int32_t heads;                     /* G query vectors per adapter */
  const void* query[2];              /* f32 [768]: emotion_q, cause_q */
  const void* q_w[2]; const void* q_b[2];
  const void* k_w[2];
  const void* v_w[2]; const void* v_b[2];
  const void* o_w[2]; const void* o_b[2];
  void* u;                           /* f32 [2, G, 768]: written by carel_adapter_build_u, read by forward and backward */
  const void* x_f32;                 /* f32 [Bp*S, 768] last hidden states (carel_encoder_x_last, dense rows) */
  void* out_f32;                     /* f32 [2, B, 768] adapter outputs (= carel_tail_args.head_in_f32) */
  const void* d_out_f32;             /* f32 [2, B, 768] (backward; = carel_tail_args.d_head_in_f32) */
  void* dx_f32;                      /* f32 [Bp*S, 768] (backward): d loss / d H, every row written (the encoder backward's dx) */
  void* work;                        /* f32 [carel_adapter_workspace_floats(B, S, G)]; the forward leaves p there for the backward */
} carel_adapter_args;
int64_t carel_adapter_workspace_floats(int32_t batch, int32_t seq_len, int32_t heads);
/* u from query / q_* / k_w (a GEMV and a transposed GEMV per adapter).  Call whenever the queries or those weights changed. */
int carel_adapter_build_u(const carel_adapter_args* args, void* stream);
/* out (and p in work) from x and u */
int carel_adapter_forward(const carel_adapter_args* args, void* stream);
/* dx from d_out, x, u and the p of the preceding forward:  dctx = d_out (modes 1 / 2) or W_v,h^T (W_o^T d_out)_h (raw);
 * dp[h,s] = H_s . dctx_h;  dz = normaliser backward (softmax p(dp - sum p dp), evaluated with dp shifted by its value at the
 * largest p so that a one-hot row does not cancel; sparsemax dp - mean_support dp on p > 0; entmax15 g dp - (sum g dp / sum g) g with g = sqrt(p));  dH_s = sum_adapters sum_h p[h,s] dctx_h + dz[h,s] u_h.
 * Adapter weight gradients are not formed (the reference never applies them: its get_params() leaves the adapters out, :460). */
int carel_adapter_backward(const carel_adapter_args* args, void* stream);

/* Adapter weight gradients (opt-in: the reference never trains its adapters, so nothing on the reference-parity path calls this).
 * Call after carel_adapter_forward and carel_adapter_backward with the SAME carel_adapter_args.  The regions of args->work those
 * calls left must be intact: qv = W_q e + b_q (carel_adapter_build_u), p (forward), dp (the backward's rowdot, in the score region)
 * and, raw mode, ctx / vcat (forward) and dvcat (backward); args->u, x_f32, d_out_f32, query and k_w are read too.  Nothing of
 * args->work, dx_f32 or out_f32 is written.  With c = 1/sqrt(768/G), head(n) = n / (768/G), e the fixed query:
 *   dz[h,b,s]  the normaliser backward, recomputed from p and dp by the expressions of carel_adapter_backward
 *   du_h       = c * sum_b sum_s dz[h,b,s] H[b,s]      (one pass over H: per-sample partials, then the samples in ascending order)
 *   dqv[n]     = W_k[n,:] . du_head(n)                  d_k_w[n,:] = qv[n] du_head(n)        d_k_b = 0 (translation invariance)
 *   d_q_w      = dqv (x) e                              d_q_b = dqv
 *   raw only:  d_o_w = sum_b d_out[b] (x) vcat[b]       d_o_b = sum_b d_out[b]
 *              d_v_w[n,:] = sum_b dvcat[b][n] ctx_head(n)[b]                                 d_v_b[n] = sum_b dvcat[b][n]
 * The queries e get no gradient (b_q already makes qv arbitrary).  f32, every sum in a fixed order, no atomics: a repeated call
 * gives the same bits.  Destinations per adapter (0 = emotion, 1 = cause), [768, 768] row-major / [768]; d_v_* / d_o_* are read in
 * raw mode only (may be NULL otherwise).  accumulate: 0 = overwrite, 1 = add to what the destinations hold. */
typedef struct carel_adapter_wgrad_args {
  void* d_q_w[2]; void* d_q_b[2];
  void* d_k_w[2]; void* d_k_b[2];
  void* d_v_w[2]; void* d_v_b[2];
  void* d_o_w[2]; void* d_o_b[2];
  void* work;                        /* f32 [carel_adapter_wgrad_workspace_floats(B, G)]: its own scratch, apart from carel_adapter_args.work */
  int32_t accumulate;
} carel_adapter_wgrad_args;
int64_t carel_adapter_wgrad_workspace_floats(int32_t batch, int32_t heads);
int carel_adapter_backward_weights(const carel_adapter_args* args, const carel_adapter_wgrad_args* grads, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused Adam over a flat parameter buffer.  Replaces torch.optim.Adam(...).step() (ref :936, :842) with
 * torch's defaults and update order (lerp for exp_avg; sqrt(v)/sqrt(bc2) + eps).  Optionally refreshes
 * the bf16 shadow copy the GEMMs read.  [skip_lo, skip_hi) is left untouched when *skip_flag != 0
 * (the pair head when its loss term was replaced by 0, ref :510-511, has grad None in the reference).
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_adam_args {
  void* param; const void* grad; void* exp_avg; void* exp_avg_sq;   /* f32 [n], 16-byte aligned */
  void* shadow_bf16;                                                 /* bf16 [n] or NULL; 8-byte aligned (stored four at a time) */
  int64_t n;
  int64_t step;                       /* 1-based step count (bias correction) */
  float lr, beta1, beta2, eps;
  float grad_scale;                   /* multiplies the gradient first (0 = 1.0) */
  int64_t skip_lo, skip_hi; const void* skip_flag;
  /* AdamW / clipping (the sentence-transformer fine-tune, fit(): AdamW weight_decay 0.01 on weight matrices only,
   * max_grad_norm 1): all optional, zero / NULL = plain Adam */
  const void* grad_scale_dev;         /* device f32 scalar multiplied into the gradient as well (carel_grad_norm_clip's coefficient) */
  float weight_decay;                 /* decoupled: param *= 1 - lr * weight_decay before the update, inside decay_segments */
  const void* decay_segments;         /* device int64 [n_decay_segments][2]: sorted [start, end) element ranges relative to
                                         `param` (multiples of 4) */
  int32_t n_decay_segments;
  /* optional device f32 scalar owned by the caller (zero it once): how many steps [skip_lo, skip_hi) has been frozen so far.
   * The range's bias corrections then use step - *skip_count (torch.optim.Adam advances a parameter's step counter only
   * when it has a gradient), and the call adds 1 to it when *skip_flag != 0. */
  void* skip_count;
} carel_adam_args;
int carel_adam_step(const carel_adam_args* args, void* stream);
int carel_cast_f32_to_bf16(const void* src_f32, void* dst_bf16, int64_t n, void* stream);
/* torch.optim.RMSprop(params, lr).step() with torch's defaults (alpha 0.99, eps 1e-8, no momentum, not centered): the
 * optimiser of the five discriminators of drl_classifier_en.py (:1056-1060).  fp32 only (the discriminators have no bf16 copy). */
int carel_rmsprop_step(void* param_f32, const void* grad_f32, void* square_avg_f32, int64_t n, float lr, float alpha, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sentence-embedding fine-tuning (chi_ec_sentence_transformer.py / en_ec_sentence_transformer.py :22, :78, :84-87; the
 * arithmetic is in the third-party `sentence_transformers`, absent here: parity unpinned, oracle/carel_oracle_st.py restates
 * the published algorithm).  fp32.
 *   carel_mean_pool_*: Pooling(mode "mean") over the attended tokens of the last hidden states x f32 [rows, hidden]:
 *     sample b owns rows row0[b] .. row0[b] + len[b] (prefix-form masks); backward writes EVERY row of dx (zeros outside).
 *   carel_triplet_semihard: losses.BatchSemiHardTripletLoss(model, margin), Euclidean distance, forward and (demb != NULL)
 *     the gradient w.r.t. the embeddings for upstream gradient 1; batch <= 64; labels int32.
 *   carel_grad_norm_clip: out2 = {||grad||_2, min(1, max_norm / (norm + 1e-6))} (torch.nn.utils.clip_grad_norm_);
 *     scratch = 1024 floats; pass out2 + 1 as carel_adam_args.grad_scale_dev.
 *   carel_l2_normalize_*: models.Normalize (the third module of all-mpnet-base-v2): y = x / max(||x||_2, 1e-12) per row; norm f32
 *     [rows] is saved for the backward dx = (g - y (y . g)) / norm.
 * ---------------------------------------------------------------------------------------------- */
int carel_mean_pool_fwd(const void* x_f32, const void* row0_i32, const void* len_i32, int32_t batch, int32_t hidden, void* out_f32, void* stream);
int carel_mean_pool_bwd(const void* g_f32, const void* row_sample_i32, const void* len_i32, int64_t rows, int32_t hidden, void* dx_f32, void* stream);
int carel_triplet_semihard(const void* emb_f32, const void* labels_i32, int32_t batch, int32_t hidden, float margin, void* loss_out_f32,
                           void* demb_f32, void* stream);
int carel_grad_norm_clip(const void* grad_f32, int64_t n, float max_norm, void* scratch_f32, void* out2_f32, void* stream);
int carel_l2_normalize_fwd(const void* x_f32, int32_t rows, int32_t hidden, void* y_f32, void* norm_f32, void* stream);
int carel_l2_normalize_bwd(const void* g_f32, const void* y_f32, const void* norm_f32, int32_t rows, int32_t hidden, void* dx_f32, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The batch triplet loss family of `sentence_transformers` (losses.BatchSemiHardTripletLoss, BatchAllTripletLoss -- the loss of
 * chi_sentence_transformer_old.py:33 --, BatchHardTripletLoss, BatchHardSoftMarginTripletLoss) for 1 <= batch <= 512: forward and
 * (demb != NULL) the gradient w.r.t. the embeddings for upstream gradient 1.  Parity unpinned (the package is absent); the
 * definitions below are restated in float64 by tests/triplet_restate.py.  fp32, no float atomics: the same inputs give the same bits.
 *   D [B, B]: distance 0 (Euclidean): d2 = |e_i|^2 - 2 e_i.e_j + |e_j|^2, D = 0 where d2 <= 0 or i == j (no gradient there), else
 *     sqrt(d2); distance 1: D = 1 - e_i.e_j, the diagonal included (the cosine distance of the package when the caller has
 *     L2-normalised the rows: carel_l2_normalize_fwd / _bwd).  D[i][j] and D[j][i] hold the same bits.
 *   pos(a, j): labels equal and j != a; neg(a, j): labels differ.  Among exactly equal distances the lowest index is selected.
 *   mode 0 semi-hard: per (a, p) the negative distance is the smallest D[a][n] > D[a][p], else the largest D[a][n], else 0 (no
 *     negative: no gradient); loss = sum max(D[a][p] - Dneg + margin, 0) / #positive pairs (0 when there is none).
 *   mode 1 all: l = D[a][p] - D[a][n] + margin over every valid (a, p, n); loss = sum max(l, 0) / (P + 1e-16), P = #{max(l, 0) > 1e-16}.
 *   mode 2 hard: hp = max_j (pos ? D[a][j] : 0), hn = min_j (D[a][j] + (neg ? 0 : max_k D[a][k])); loss = mean_a max(hp - hn + margin, 0).
 *   mode 3 hard soft-margin: the same hp, hn; loss = mean_a log1p(exp(hp - hn)) computed as a stable softplus; margin is ignored.
 *   stats_out (optional): {positive pairs, valid triplets, active terms}: active = hinge terms > 0 (mode 0: pairs, mode 2: anchors),
 *     P (mode 1), batch (mode 3).
 *   work: f32 [carel_triplet_workspace_floats(batch)], owned by the caller, fully rewritten by every call.  Afterwards
 *     work[0 .. B*B) holds D and work[B*B .. 2*B*B) holds W = d (sum of the loss terms) / d D (integer counts in the hinge modes).
 * Four launches (three without demb) on `stream`; no allocation, no host synchronisation.  Errors before any launch: a NULL
 * struct / emb / labels / loss_out / work, mode outside 0..3, distance outside 0..1 -> CAREL_ERR_ARG; batch outside 1..512 or
 * hidden < 1 -> CAREL_ERR_SHAPE.  carel_triplet_workspace_floats is a pure host function (0 for a batch outside 1..512).
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_triplet_args {
  const void* emb;      /* f32 [batch, hidden], contiguous */
  const void* labels;   /* int32 [batch] */
  int32_t batch, hidden;
  int32_t mode;         /* 0 semi-hard, 1 all, 2 hard, 3 hard soft-margin */
  int32_t distance;     /* 0 Euclidean, 1 one minus dot product */
  float margin;
  void* loss_out;       /* f32 [1] */
  void* demb;           /* f32 [batch, hidden] or NULL */
  void* stats_out;      /* int32 [3] or NULL */
  void* work;           /* f32 [carel_triplet_workspace_floats(batch)] */
} carel_triplet_args;
int64_t carel_triplet_workspace_floats(int32_t batch);
int carel_triplet_loss(const carel_triplet_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RBF-MMD statistic.  Replaces MMDStatistic.__call__ (ref :547-569) + pdist (ref :580-589) and
 * their autograd backward.  mmd = 2*a01*sum(K12) + a00*(sum(K11)-tr K11) + a11*(sum(K22)-tr K22),
 * K = sum_alpha exp(-alpha * (eps + |d2|)), a00 = 1/(n1(n1-1)), a11 = 1/(n2(n2-1)), a01 = -1/(n1 n2).
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_mmd_args {
  const void* s1;       /* f32 [n1, d], row stride ld1 */
  const void* s2;       /* f32 [n2, d], row stride ld2 */
  int64_t ld1, ld2;
  int32_t n1, n2, d;    /* d <= 64 */
  int32_t n_alphas;     /* 1..8 */
  float alphas[8];
  float eps;            /* 1e-5 in the reference */
  void* mmd_out;        /* f32 [1] */
  void* kernels_out;    /* optional f32 [(n1+n2)^2]  (ret_matrix=True) or NULL */
  /* backward only: */
  const void* grad_mmd; /* f32 [1] upstream gradient */
  void* g1;             /* f32 [n1, d] contiguous: d mmd / d s1 * grad */
  void* g2;             /* f32 [n2, d] contiguous */
} carel_mmd_args;

int carel_rbf_mmd_fwd(const carel_mmd_args* args, void* stream);
int carel_rbf_mmd_bwd(const carel_mmd_args* args, void* stream);

/* The kernel matrix alone, tiled: kernels_out f32 [(n1+n2)^2] of the same struct (mmd_out and the backward fields are not read), each
 * element by the expression carel_rbf_mmd_fwd evaluates, sum_a expf(-alpha_a * (eps + |d2|)), so the matrix is bitwise symmetric.
 * Any n1, n2 >= 1 with n1 + n2 <= 8192 (carel_rbf_mmd_fwd keeps both samples in one workgroup's LDS and stops near 1 600 rows at d = 24;
 * this one holds 128 rows per workgroup whatever n is), d in 1..64, 1..8 alphas, row strides >= d.  One launch.  Errors before it:
 * a NULL struct / sample / kernels_out, n_alphas outside 1..8, a row stride below d -> CAREL_ERR_ARG; the shape -> CAREL_ERR_SHAPE. */
int carel_rbf_gram(const carel_mmd_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Permutation two-sample test on a kernel matrix: the body of MMDStatistic.pval / permutation_test_mat.  The reference's function
 * is a stub (ref :599-600) and the package it came from is not at hand, so this DEFINITION IS THE PROJECT'S OWN (parity unpinned):
 *   M f32 [n, n], n = n1 + n2, not necessarily symmetric, diagonal never read as a value (a NaN there changes nothing);
 *   for a labelling g in {0,1}^n:  stat(g) = sum over i != j of c(g_i, g_j) M_ij,  c(0,0) = a00, c(1,1) = a11, c(0,1) = c(1,0) = a01;
 *   labels u8 [P+1, n] contiguous, row 0 = the observed labelling [0]*n1 + [1]*n2 (with MMDStatistic's coefficients stat(row 0) is
 *   what __call__ returns), rows 1..P the relabellings -- any 0 / non-zero bytes: the CALLER sees to it that each row holds n2 ones;
 *   stats f64 [P+1] = stat of every row;  count i32 [1] = #{p in 1..P : stats[p] >= stats[0]}, compared on the doubles on the device;
 *   p-value = count / P (the observed labelling is not among the P).
 * The f32 arithmetic is a chain of at most 32 additions per partial sum; everything after it is double, in an order fixed by indices:
 * equal rows of `labels` give equal bits wherever they stand, and so do two runs (csrc/mmd_perm.hip; the bound: tests/perm_restate.py).
 * workspace: carel_mmd_perm_workspace_bytes(n, P) bytes of device memory (8-byte aligned), fully rewritten by every call; the
 * function is pure host code and returns 0 for a shape outside the limits.
 * Limits: n1, n2 >= 2, n <= 8192, 1 <= P <= 65535, ldm >= n.  Four launches on `stream`, no allocation, no host synchronisation.
 * Errors before the first launch: a NULL struct / matrix / labels / stats / count / workspace, ldm < n, a workspace smaller than
 * stated -> CAREL_ERR_ARG; n1, n2, n or P outside the limits -> CAREL_ERR_SHAPE.
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_mmd_perm_args {
  const void* matrix;       /* f32 [n, n], row stride ldm */
  int64_t ldm;
  const void* labels;       /* u8 [P+1, n] */
  int32_t n1, n2;
  int32_t n_permutations;   /* P */
  double a00, a01, a11;
  void* stats;              /* f64 [P+1] */
  void* count;              /* i32 [1] */
  void* workspace;
  int64_t workspace_bytes;
} carel_mmd_perm_args;
int64_t carel_mmd_perm_workspace_bytes(int32_t n, int32_t n_permutations);
int carel_mmd_perm_test(const carel_mmd_perm_args* args, void* stream);

/* z f32 [n, 2*ec_dim] = [mu_e + eps_e * exp(lv_e) | mu_c + eps_c * exp(lv_c)] of every row of lat f32 [n, 4*ec_dim] (the output of
 * carel_tail_latents) with ONE noise pair eps_e, eps_c f32 [ec_dim]: the samples that carel_pair_probs / draw 0 of
 * carel_pair_probs_draws feed to the pair head, written out (the two-sample test on a model's latents).  ec_dim in 1..32, n >= 1. */
int carel_sample_latents(const void* lat, const void* eps_e, const void* eps_c, int32_t n, int32_t ec_dim, void* z, void* stream);

/* Replaces `pdist(sample_1, sample_2, norm=2, eps)` (ref :580-589, the live L2 branch) and its autograd backward:
 * dist[i][j] = sqrt(eps + |  |s1_i|^2 + |s2_j|^2 - 2 s1_i . s2_j  |), computed from the squared distance itself (no
 * exp / log round trip), so far-apart samples (d2 >> 100) and near-coincident ones are both exact to fp32 rounding. */
typedef struct carel_pdist_args {
  const void* s1;       /* f32 [n1, d], row stride ld1 */
  const void* s2;       /* f32 [n2, d], row stride ld2 */
  int64_t ld1, ld2;
  int32_t n1, n2, d;    /* d <= 64 */
  float eps;            /* 1e-5 in the reference */
  void* dist_out;       /* fwd: f32 [n1, n2] */
  const void* grad_dist;/* bwd: f32 [n1, n2] upstream gradient */
  void* g1;             /* bwd: f32 [n1, d] contiguous */
  void* g2;             /* bwd: f32 [n2, d] contiguous */
} carel_pdist_args;
int carel_pdist_fwd(const carel_pdist_args* args, void* stream);
int carel_pdist_bwd(const carel_pdist_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * HSIC statistic (ablation head).  Replaces HSIC / GaussianKernelMatrix / pairwise_distances of
 * drl_classifier_ec_hsic.py:529-547 and their backward: tr(L H K H)/(m-1)^2, K = exp(-D(x)/s_x),
 * L = exp(-D(y)/s_y), D = squared Euclidean distances, H = I - 11^T/m.
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_hsic_args {
  const void* x; const void* y;     /* f32 [m, d], row strides ldx / ldy */
  int64_t ldx, ldy;
  int32_t m, d;                     /* d <= 64 */
  float s_x, s_y;                   /* 1 in the reference */
  void* hsic_out;                   /* f32 [1] */
  const void* grad_hsic;            /* bwd: f32 [1] upstream gradient (NULL = 1) */
  void* gx; void* gy;               /* bwd: f32 [m, d] contiguous */
} carel_hsic_args;
int carel_hsic_fwd(const carel_hsic_args* args, void* stream);
int carel_hsic_bwd(const carel_hsic_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The two differentiable statistics on samples of up to 8192 rows (csrc/stat_tiled.hip, stat_tiled_device.h).  carel_hsic_fwd/bwd and
 * carel_rbf_mmd_fwd/bwd keep both samples in one workgroup's LDS and stop there (HSIC m = 757 at d = 24, MMD n1 + n2 = 1572); these
 * take the same structs, evaluate element by element the same expressions (hsic_kern of csrc/hsic_device.h, mmd_pair_kernel of
 * csrc/mmd_device.h; the centred coefficients of hsic_backward_row, the weights of mmd_backward_row) and differ in the order of the
 * sums only: workgroups own 64 x 64 tiles of rows x partner rows, neither matrix is stored, LDS per workgroup is below 64 KB whatever
 * the sample size.  A thread adds 16 kernel values in float; everything across threads and tiles (the three HSIC sums, the row sums RK_i,
 * RL_i, TK, TL; the three MMD block sums) is added in double in an order fixed by indices and rounded once.  A gradient element is a
 * float chain over the partners of one run of tiles, then the runs in turn.  No atomics: two calls give the same bits.
 *   HSIC  2 <= m <= 8192;   MMD  n1, n2 >= 2, n1 + n2 <= 8192;   1 <= d <= 64, row strides >= d, 1..8 alphas, widths > 0.
 *   grad_hsic / grad_mmd NULL = an upstream gradient of 1.  kernels_out of carel_mmd_args is NOT read by the tiled entries
 *   (carel_rbf_gram writes the matrix).  The forward entries write hsic_out / mmd_out only, the backward entries gx, gy / g1, g2 only.
 *   work: carel_hsic_tiled_workspace_bytes(m, d) / carel_rbf_mmd_tiled_workspace_bytes(n1, n2, d) bytes of device memory, 8-byte
 *   aligned, rewritten by every call; with T = ceil(rows / 64), S = ceil(T / ceil(T / min(T, max(1, 1024 / T)))) (integer division):
 *     HSIC  8 (T^2 + 3 ceil(m / 256)) + 4 (4 + 2 * 64 T + 2 T * 64 T + 2 S m d)        MMD  8 * 3 T^2 + 4 S (n1 + n2) d
 *   Both are pure host functions and return 0 for a shape outside the limits.
 * HSIC: three launches forward, six backward; MMD: two and two.  No allocation, no host synchronisation.  Every check comes before
 * the first launch: a NULL struct / sample / output / workspace, a misaligned workspace, a row stride below d, a width <= 0,
 * n_alphas outside 1..8 -> CAREL_ERR_ARG; m, n1, n2 or d outside the limits -> CAREL_ERR_SHAPE; the message names the entry point.
 * ---------------------------------------------------------------------------------------------- */
int64_t carel_hsic_tiled_workspace_bytes(int32_t m, int32_t d);
int carel_hsic_tiled_fwd(const carel_hsic_args* args, void* work, void* stream);
int carel_hsic_tiled_bwd(const carel_hsic_args* args, void* work, void* stream);
int64_t carel_rbf_mmd_tiled_workspace_bytes(int32_t n1, int32_t n2, int32_t d);
int carel_rbf_mmd_tiled_fwd(const carel_mmd_args* args, void* work, void* stream);
int carel_rbf_mmd_tiled_bwd(const carel_mmd_args* args, void* work, void* stream);

/* The Gram matrix of HSIC alone, tiled: k_out[i][j] = K_ij = exp(-D(x)_ij / s) f32 [m, m] (row stride ldk >= m; the padding is not
 * written), each element by the expression carel_hsic_fwd evaluates (hsic_kern of csrc/hsic_device.h: the norms and the dot product by
 * the same fmaf chains, __expf(-(n_i + n_j - 2 dot) / s)), so the matrix is bitwise symmetric and its diagonal is exactly 1.
 * carel_hsic_fwd keeps both samples in one workgroup's LDS and stops at m = 757 (d = 24); this one holds 128 rows per workgroup
 * whatever m is.  1 <= d <= 64, 2 <= m <= 8192, ldx >= d, s > 0.  One launch.  Errors before it: a NULL struct / x / k_out, ldx < d,
 * ldk < m, s <= 0 -> CAREL_ERR_ARG; m or d outside the limits -> CAREL_ERR_SHAPE.  (carel_rbf_gram evaluates the MMD form,
 * sum_a exp(-alpha_a (eps + |d2|)), and cannot serve here.) */
typedef struct carel_hsic_gram_args {
  const void* x;            /* f32 [m, d], row stride ldx */
  int64_t ldx;
  int32_t m, d;
  float s;                  /* kernel width, 1 in the reference */
  void* k_out;              /* f32 [m, m], row stride ldk */
  int64_t ldk;
} carel_hsic_gram_args;
int carel_hsic_gram(const carel_hsic_gram_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Permutation independence test on two kernel matrices (Gretton et al. 2007): the HSIC value of m paired rows and the share of random
 * re-pairings whose HSIC reaches it.  The reference has no such function, so this DEFINITION IS THE PROJECT'S OWN (parity unpinned);
 * the statistic itself is the reference's HSIC (drl_classifier_ec_hsic.py:540-547).
 *   K, L f32 [m, m], row strides ldk, ldl >= m, not necessarily symmetric, diagonal included;
 *   R_i, C_j, T the row sums, column sums and total of K;  Kc_ij = K_ij - R_i/m - C_j/m + T/m^2 = (H K H)_ij;
 *   for a permutation pi of 0..m-1:  stat(pi) = sum_ij Kc_ij L[pi_i][pi_j] / (m-1)^2  (the identity on the Gram matrices of x and y:
 *   tr(L H K H) / (m-1)^2, what carel_hsic_fwd computes);
 *   perms i32 [P+1, m] contiguous, row 0 = the observed pairing (the caller sets it to the identity), rows 1..P the re-pairings.  Every
 *   index is clamped into [0, m) before it addresses anything: a row that is no permutation gives a wrong statistic, never an access
 *   outside the matrices -- the CALLER sees to it that each row is a permutation;
 *   stats f64 [P+1] = stat of every row;  count i32 [1] = #{p in 1..P : stats[p] >= stats[0]}, compared on the doubles on the device;
 *   p-value = count / P (the observed pairing is not among the P).
 * R, C, T are summed in double and Kc_ij is formed in double and rounded to f32 once; the products Kc_ij L[pi_i][pi_j] are exact in
 * double and every sum is double, in an order fixed by indices: no atomics, equal rows of `perms` give equal bits wherever they stand,
 * and so do two runs (csrc/hsic_perm.hip; the bound: tests/hsic_perm_restate.py).
 * workspace: carel_hsic_perm_workspace_bytes(m, P) bytes of device memory, 16-byte aligned, fully rewritten by every call; the
 * function is pure host code and returns 0 for a shape outside the limits.
 * Limits: 2 <= m <= 8192, 1 <= P <= 65535.  Eight launches on `stream`, no allocation, no host synchronisation.
 * Errors before the first launch: a NULL struct / k / l / perms / stats / count / workspace, ldk or ldl < m, a workspace smaller than
 * stated or not 16-byte aligned -> CAREL_ERR_ARG; m or P outside the limits -> CAREL_ERR_SHAPE.
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_hsic_perm_args {
  const void* k;            /* f32 [m, m], row stride ldk */
  int64_t ldk;
  const void* l;            /* f32 [m, m], row stride ldl */
  int64_t ldl;
  const void* perms;        /* i32 [P+1, m] */
  int32_t m;
  int32_t n_permutations;   /* P */
  void* stats;              /* f64 [P+1] */
  void* count;              /* i32 [1] */
  void* workspace;
  int64_t workspace_bytes;
} carel_hsic_perm_args;
int64_t carel_hsic_perm_workspace_bytes(int32_t m, int32_t n_permutations);
int carel_hsic_perm_test(const carel_hsic_perm_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exact order statistics of the squared pairwise distances of one sample (the median-heuristic kernel width of the two permutation
 * tests above).  The reference has no such function, so this DEFINITION IS THE PROJECT'S OWN (parity unpinned).
 *   x f32 [m, d], row stride ldx >= d;  D_ij = n_i + n_j - 2 dot_ij in float32 with the norms and the dot product by the fmaf chains
 *   of hsic_kern (csrc/hsic_device.h, hsic_sqdist): the number carel_hsic_gram multiplies by -1/s, bit for bit -- bitwise symmetric,
 *   D_ii = +0, no abs, so near-duplicate rows far from the origin can give a slightly negative value;
 *   the population is the multiset { D_ij : i < j } of N = m (m-1) / 2 values (the matrix is never stored);
 *   for each of the n_ranks ranks r (HOST values, 0-based, in [0, N), repeats allowed):  values[q] = v_r, the r-th smallest element,
 *   with the bits of one of the D_ij (a -0 is returned as +0);  counts[q] = { #{D < v_r}, #{D == v_r} }, so that
 *   counts[q][0] <= r < counts[q][0] + counts[q][1].
 * A three-pass radix select (11 / 11 / 10 bits) on an order-preserving key of the float, the distances recomputed per pass from rows
 * staged in LDS; all counting is integer (atomicAdd on integers only), so two runs give the same bits.  Precondition: finite inputs
 * (a NaN distance ranks above +inf and comes back as a NaN; no input can make an index leave a histogram).  csrc/pdist_select.hip;
 * the bound against float64: tests/pdist_select_restate.py.
 * workspace: carel_pdist_select_workspace_bytes(m, n_ranks) bytes of device memory, 16-byte aligned, fully rewritten by every call; the
 * function is pure host code and returns 0 for a shape outside the limits.
 * Limits: 2 <= m <= 8192, 1 <= d <= 64, 1 <= n_ranks <= 8.  Seven launches on `stream`, no allocation, no host synchronisation.
 * Errors before the first launch (nothing is written): a NULL struct / x / values / workspace, ldx < d, a rank outside [0, N), a
 * workspace smaller than stated or not 16-byte aligned -> CAREL_ERR_ARG; m, d or n_ranks outside the limits -> CAREL_ERR_SHAPE.
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_pdist_select_args {
  const void* x;            /* f32 [m, d], row stride ldx */
  int64_t ldx;
  int32_t m, d;
  int32_t n_ranks;
  int64_t ranks[8];         /* host values */
  void* values;             /* f32 [n_ranks] */
  void* counts;             /* i64 [n_ranks][2] = below, equal; may be NULL */
  void* workspace;
  int64_t workspace_bytes;
} carel_pdist_select_args;
int64_t carel_pdist_select_workspace_bytes(int32_t m, int32_t n_ranks);
int carel_pdist_select(const carel_pdist_select_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * VI / CLUB head (ablation script drl_classifier_ec_vi.py).  z = [e | c] f32 [B, 2*ec_dim] are the sampled emotion /
 * cause embeddings; net[8] = approximation network p(e|c): ec_mu.0.weight, ec_mu.0.bias, ec_mu.2.weight, ec_mu.2.bias,
 * ec_log_var.0.weight, .0.bias, .2.weight, .2.bias (:156-163).
 *   carel_vi_aprx : get_ec_aprx_loss (:422-427) on c.detach() -> loss_out and d_net[8] (gradients of the net only)
 *   carel_vi_upper: get_ec_upper_loss (:429-440) with negatives e[perm] -> loss_out and dz = d loss / d z [B, 2*ec_dim]
 *                   (feed it to carel_tail_backward's dz_extra, scaled by beta)
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_vi_args {
  const void* z;
  int32_t batch, ec_dim;             /* ec_dim <= 32 */
  const void* net[8];
  const void* perm;                  /* int32 [B], upper only */
  void* loss_out;                    /* f32 [1] */
  void* d_net[8];                    /* aprx only */
  void* dz;                          /* upper only, f32 [B, 2*ec_dim] (overwritten) */
} carel_vi_args;
int carel_vi_aprx(const carel_vi_args* args, void* stream);
int carel_vi_upper(const carel_vi_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Adversarial (GAN) disentangler of the two-space ablation script drl_classifier_ec_gan.py: the two one-logit
 * adversaries on the DETACHED sampled embeddings z = [e | c] f32 [B, 2*ec_dim] (:430-477)
 *   disc 0 = ec_disc: p = sigmoid(w . dropout(c) + b), scored against the EMOTION labels   (:222-225)
 *   disc 1 = ce_disc: p = sigmoid(w . dropout(e) + b), scored against the CAUSE labels     (:231-234)
 *   loss    = mean_b BCELoss(p, y (1 - label_smoothing) + label_smoothing)   (logs clamped at -100, :458-470)
 *   entropy = mean_b p log(p + epsilon)                                       (:472-477; p log p, not a binary entropy)
 * ONE launch writes terms[0..3] = ec_disc_loss, ce_disc_loss, ec_entropy, ce_entropy and, for UNIT upstream gradients
 * (the losses are roots of the graph; the caller scales), the four gradient images over [weight (ec_dim), bias]:
 *   g_loss_w/b[i] = d loss_i / d disc_i,   g_ent_w/b[i] = d entropy_i / d disc_i.
 * Because of the detach nothing here reaches z: there is no dz.  With vae_loss_in (f32 [1], the tail's terms[8]) also
 * terms[4] = *vae_loss_in + w_entropy * (ec_entropy + ce_entropy), the vae_and_classifier_loss of :275-279.
 * Dropout: the library's counter-based masks at sites 103 (ec_disc's input) and 104 (ce_disc's input), element index
 * (drop_row_offset + b) * ec_dim + k.  Every sum runs in a fixed order (no atomics): the same inputs give the same bits.
 * 1 <= batch <= 1024 (this kernel's own limit; the tail that produces z is tighter, see carel_tail_losses), 1 <= ec_dim <= 32
 * (the tail's limit).  Bad arguments return before any HIP call; nothing is allocated and the host is never synchronised.
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_gan_args {
  const void* z;                     /* f32 [B, 2*ec_dim] (carel_tail_args.z) */
  int32_t batch, ec_dim;
  const void* emo_labels;            /* f32 [B] */
  const void* cau_labels;            /* f32 [B] */
  const void* disc_w[2];             /* f32 [ec_dim]: ec_disc.weight, ce_disc.weight */
  const void* disc_b[2];             /* f32 [1] */
  float label_smoothing, epsilon;
  float drop_p; uint32_t drop_seed; uint32_t drop_row_offset;
  const void* vae_loss_in;           /* f32 [1] or NULL */
  float w_entropy;                   /* ecce_adv_loss_weight (used for terms[4] only) */
  void* terms;                       /* f32 [8]: 0..3 as above, 4 = total (with vae_loss_in), 5..7 unused */
  void* g_loss_w[2]; void* g_loss_b[2];
  void* g_ent_w[2]; void* g_ent_b[2];
} carel_gan_args;
int carel_gan_disc(const carel_gan_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tail of the three-space adversarial model of drl_classifier_en.py (config 4): replaces everything after
 * `pooler_output` in DrlClassifier.forward (drl_classifier_en.py:220-334) and the gradient side of the six
 * backward calls of its training step (:919-939).  fp32 throughout.
 *
 * Latent layout  lat [B, 2*con_dim + 4*ec_dim] = content_mu | content_log_var | emotion_mu | emotion_log_var |
 *                                                cause_mu | cause_log_var               (:227-232, :378-415)
 * Sample layout  z   [B, 2*ec_dim + con_dim]   = emotion | cause | content  == generative_emb (:243);
 *                eps  [2*ec_dim + con_dim] in the same layout (the reference draws content, emotion, cause in that
 *                order, :238-240 -- the caller fills eps accordingly).
 * terms [32]: 0..6 = content_disc_loss_emo, content_disc_loss_cau, emotion_disc_loss, ec_disc_loss,
 *             cause_disc_loss, ce_disc_loss, vae_and_classifier_loss (the tuple forward returns, :334);
 *             7,8 content entropies (emo, cau); 9 emotion_disc entropy; 10 cause_disc entropy; 11 ec_disc entropy;
 *             12 ce_disc entropy; 13 emo_mul; 14 cau_mul; 15 content_mul; 16 pair_mul; 17 kl_e; 18 kl_c;
 *             19 kl_content (the three already multiplied by their annealed weights); 20 reconstruction.
 *
 * Every discriminator reads a DETACHED embedding (:425-515), so its loss and its entropy term reach only its own
 * parameters.  carel_en_tail_losses writes, for unit upstream gradients:
 *   g_cdisc_*[0], [1] : d content_disc_loss_emo / d content_disc, d content_disc_loss_cau / d content_disc
 *   g_cdisc_*[2]      : d vae_loss / d content_disc   (= con_adv_weight * both entropies)
 *   g_sdisc_*[i]      : d (own discriminator loss) / d {emotion_disc, cause_disc, ec_disc, ce_disc}[i]
 *   g_sdisc_ent_*[i]  : d vae_loss / d the same (weighted entropy)
 *   d_*               : d vae_loss / d {content_classifier, emotion/cause/pair classifier, decoder}
 * and keeps d vae_loss / d lat in `work`; carel_en_tail_backward turns that into d_pooler_* and dx_last, all
 * scaled by *grad_out_dev.  The six latent heads are not in any optimiser group (:357-376): no gradient is
 * produced for them.  Dropout masks: counter-based, sites 110..119 in the order of the ten nn.Dropout calls.
 * ---------------------------------------------------------------------------------------------- */
typedef struct carel_en_tail_args {
  int32_t batch, seq_len, hidden, ec_dim, con_dim, bow_dim;
  const void* x_last_f32;            /* f32 [rows, 768] last encoder LayerNorm output */
  const void* cls_rows;              /* int32 [B] or NULL (= b*seq_len) */
  int32_t n_rows;                    /* rows of dx_last to clear (0 = B*seq_len) */
  const void* pooler_w; const void* pooler_b;
  const void* head_w[6]; const void* head_b[6];     /* content_mu, content_log_var, emotion_mu, emotion_log_var, cause_mu, cause_log_var */
  const void* cdisc_w; const void* cdisc_b;         /* content_disc [V, ec_dim] */
  const void* sdisc_w[4]; const void* sdisc_b[4];   /* emotion_disc [1,con_dim], cause_disc [1,con_dim], ec_disc [1,ec_dim], ce_disc [1,ec_dim] */
  const void* ccls_w; const void* ccls_b;           /* content_classifier [V, con_dim] */
  const void* emo_w; const void* emo_b; const void* cau_w; const void* cau_b;   /* [1, ec_dim] */
  const void* pair_w; const void* pair_b;           /* [1, 2*ec_dim] */
  const void* dec_w; const void* dec_b;             /* [V, 2*ec_dim + con_dim] */
  const void* emo_labels; const void* cau_labels; const void* pair_labels;     /* f32 [B] */
  const void* bow;                                  /* f32 [B, V] */
  const void* eps;                                  /* f32 [2*ec_dim + con_dim] */
  float w_con_adv, w_ec_adv, w_ecce_adv, w_ec_mul, w_con_mul, w_pair;           /* :325-330 */
  float kl_w_ec, kl_w_con;                          /* annealed KL weights (1 once iteration >= kl_ann_iterations) */
  float label_smoothing, epsilon;
  float drop_p; uint32_t drop_seed;
  uint32_t drop_row_offset;                         /* data parallel: first GLOBAL sample index of this shard (dropout masks hash
                                                       the global element index) */
  const void* global_label_sum;                     /* f32 [1] or NULL: sum of pair labels over the GLOBAL batch (pos_weight, :599) */
  int32_t global_n;                                 /* global batch size (with global_label_sum) */
  /* outputs */
  void* pooled;                      /* f32 [B, 768] */
  void* lat;                         /* f32 [B, 2*con_dim + 4*ec_dim] */
  void* z;                           /* f32 [B, 2*ec_dim + con_dim] */
  void* terms;                       /* f32 [32] */
  void* work;                        /* f32 [carel_en_tail_workspace_floats(...)] */
  void* g_cdisc_w[3]; void* g_cdisc_b[3];
  void* g_sdisc_w[4]; void* g_sdisc_b[4];
  void* g_sdisc_ent_w[4]; void* g_sdisc_ent_b[4];
  void* d_ccls_w; void* d_ccls_b; void* d_emo_w; void* d_emo_b; void* d_cau_w; void* d_cau_b;
  void* d_pair_w; void* d_pair_b; void* d_dec_w; void* d_dec_b;
  void* d_pooler_w; void* d_pooler_b;
  void* dx_last_f32;                 /* f32 [n_rows, 768] */
} carel_en_tail_args;
int64_t carel_en_tail_workspace_floats(int32_t batch, int32_t ec_dim, int32_t con_dim, int32_t bow_dim);
int carel_en_tail_latents(const carel_en_tail_args* args, void* stream);     /* pooled, lat (also the front of get_pair_preds, :336-349) */
int carel_en_tail_losses(const carel_en_tail_args* args, void* stream);      /* z, terms and every gradient listed above */
int carel_en_tail_backward(const carel_en_tail_args* args, const void* grad_out_dev_f32, void* stream);
/* The same tail with the ELEMENT-WEIGHTED content losses of drl_classifier_bow_loss.py (:245-257, :438-448, :537-550):
 *   con_w = sigmoid(content_classifier(dropout(z_content)))        [B, V]; its own dropout draw, DETACHED
 *   content_disc_loss_{emo,cau} = BCELoss(weight = 1 - con_w)(softmax(content_disc(dropout(z_{e,c}))), smoothed_bow)
 *   content_mul_loss            = BCELoss(weight = con_w)    (softmax(content_classifier(dropout(z_content))), smoothed_bow)
 * With p the softmax row, t the smoothed target and omega the weight, the row statistic is sum_j omega_j * bce_j (both logs
 * clamped at -100 before the multiply, as nn.BCELoss does), reduced by the plain mean over B * V (not by sum omega), and
 *   d loss / d logit_j = p_j * (omega_j * g_j - sum_k p_k * omega_k * g_k) / (B * V),   g = (p - t) / (p * (1 - p)).
 * The weight is a constant: nothing flows into content_classifier or z_content through it.  Entropies, decoder, one-logit
 * heads, KL terms and the weighted sum are those of carel_en_tail_losses, bit for bit; terms[], every gradient image and
 * `work` have the same meaning, so carel_en_tail_backward follows unchanged.
 * The weight input is an eleventh dropped-out copy of the content sample at dropout SITE 120 (sites 110..119 keep their
 * meaning; drop_row_offset applies to it like to the others).  One fp32 GEMM [B, con_dim] x [con_dim, V] and one
 * element-wise pass write con_w ONCE into the scratch below; the row passes of the three heads read it.
 * Errors before any launch: NULL `bow` / `bow->work` -> CAREL_ERR_ARG; a shape outside carel_en_tail_losses' range
 * (batch 1..1024, ...) -> CAREL_ERR_SHAPE. */
typedef struct carel_en_bow_args {
  void* work;                        /* f32 [carel_en_tail_bow_workspace_floats(...)]: site-120 copy [B, con_dim], then con_w [B, V] */
} carel_en_bow_args;
int64_t carel_en_tail_bow_workspace_floats(int32_t batch, int32_t con_dim, int32_t bow_dim);
int carel_en_tail_losses_bow(const carel_en_tail_args* args, const carel_en_bow_args* bow, void* stream);
/* get_pair_preds (:336-353): raw pair logits from lat with fresh emotion / cause noise (f32 [ec_dim] each) */
int carel_en_pair_logits(const void* lat, int32_t lat_stride, int32_t emo_off, int32_t cau_off, const void* eps_e, const void* eps_c,
                         const void* pair_w, const void* pair_b, int32_t batch, int32_t ec_dim, void* logits, void* stream);
/* dst = (accumulate ? dst : 0) + *scale_dev * src   (scale_dev NULL = 1): how a discriminator's .grad takes one
 * backward call's share without a host sync */
int carel_axpy_f32(void* dst_f32, const void* src_f32, int64_t n, const void* scale_dev_f32, int32_t accumulate, void* stream);
/* fp32 GEMM used by the vocabulary-wide heads (exposed for the parity tests): C[M,N] (+)= op(A) op(B)
 * ta = 0: A is [M,K] row-major (lda); 1: A is [K,M].  tb = 0: B is [N,K] row-major (ldb); 1: B is [K,N].
 * bias [N] or NULL.  splits > 1: C receives `splits` partial results c_split_stride floats apart (no bias). */
int carel_sgemm_f32(const void* A, int64_t lda, int32_t ta, const void* B, int64_t ldb, int32_t tb, void* C, int64_t ldc,
                    int32_t M, int32_t N, int32_t K, const void* bias, int32_t accumulate, int32_t splits, int64_t c_split_stride,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Hardware-layout self test (MFMA fragment maps, transposed LDS reads, LDS-DMA staging) used by
 * tests/test_gpu_layouts.py: raw dumps of what the helpers produce on exact integer data (layout of
 * the two buffers is documented in csrc/selftest.hip); the test compares them with numpy.
 * ---------------------------------------------------------------------------------------------- */
int carel_selftest_layouts(const void* in_bf16_40960, void* out_f32_73728, void* stream);

#ifdef CAREL_EXPERIMENTS
#include "carel_hip_experiments.h"
#endif
#ifdef __cplusplus
}
#endif
#endif /* CAREL_HIP_H */
