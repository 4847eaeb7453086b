/* espresso_amd — C ABI of the MI355X (gfx950) hot path of freewym/espresso.
 *
 * The reference has no FFI on this path: its boundary is fairseq's Python plugin registry
 * (SURVEY.md §8b), and all compute below it is ATen/cuDNN/torchaudio calls.  This header is the
 * boundary this framework introduces UNDER that registry: one entry point per reference
 * function on the hot path, plain device pointers + sizes + a HIP stream, no torch types.  The
 * host-side mirror of the reference interface (espresso_amd/{data,modules,models,criterions,
 * tasks,tools}) binds these through ctypes (espresso_amd/_lib.py); INTEGRATION.md shows the stub
 * a reference maintainer would add.  Each declaration cites the reference code it replaces
 * (paths relative to the reference root).
 * Entry points without a counterpart in the reference say so where they are declared: the streaming
 * kernels (ea_stream_*) and the causal depthwise convolution of the Conformer convolution module
 * (ea_glu_dwconv_causal_*, ea_dwconv_causal_bwd_weight, EaLayerShape.conv_causal, ea_stream_glu_dwconv_bn_act), which
 * exists so that a Conformer encoder can be streamed: the reference's module pads symmetrically.
 *
 * Conventions: every function returns 0 on success, a negative value on a launch/argument
 * error; all pointers are DEVICE pointers unless the name ends in _host; `stream` is a
 * hipStream_t (0 = default stream); kernels are asynchronous with respect to the host.
 * bf16 tensors are raw uint16 bit patterns.  "TBC" = (time, batch, channel) row-major.
 */
#ifndef ESPRESSO_AMD_H
#define ESPRESSO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* ea_stream_t;

int ea_version(void);

/* ------------------------------------------------------------------------------------------
 * Dense products (MFMA).  Replaces torch.nn.functional.linear / torch.bmm / conv1d(k=1) /
 * im2col-conv2d calls at: fairseq/modules/conformer_layer.py:79-101,134-146;
 * fairseq/modules/multihead_attention.py:650-688,788-831,884-907;
 * espresso/models/transformer/speech_transformer_encoder.py:341-343;
 * espresso/models/transformer/speech_transformer_encoder_model.py:207-208;
 * espresso/modules/speech_convolutions.py:78-102.
 *
 *   C[z][m][n] = epi( alpha * sum_k A(z;m,k) * B(z;n,k) ),  z in [0,batch)
 *   A(z;m,k) = A[(z/zdiv)*sA_hi + (z%zdiv)*sA_lo + (a_kstrided ? k*lda + m : m*lda + k)]  (bf16)
 *   B likewise with n.                                                                    (bf16)
 *   epi(v):  v += bias[n]
 *            if aux:  v *= keep(drop) * act'(aux[m][n])                 (backward through act)
 *            elif C2: C = bf16(v);  C2 = bf16(keep(drop) * act(v));     (two outputs) done
 *            else:    v = keep(drop) * act(v)
 *            v = v * out_scale + resid[m][n]
 *            C = c_f32 ? (accumulate ? C + v : v) : bf16(v)
 *   splitk > 1: two-pass split-K (fp32 slabs + reduce) for wgrad: long reduction, few output tiles.
 */
enum { EA_ACT_NONE = 0, EA_ACT_RELU = 1, EA_ACT_SILU = 2 };

typedef struct EaGemmParams {
  const void* A;
  const void* B;
  void* C;
  void* C2;           /* optional bf16 second output, leading dim ldc2, same batch offsets as C */
  const float* bias;  /* [N] fp32 or NULL */
  const void* resid;  /* bf16 (or fp32 if resid_f32) [M][ldr] or NULL */
  const void* aux;    /* bf16 pre-activation [M][ldaux] or NULL */
  int M, N, K, batch, zdiv;
  int a_kstrided, b_kstrided, c_f32, accumulate, resid_f32, act;
  /* Row pitches in elements.  CONTRACT for ldc > N (a padded output pitch): the columns N .. ldc - 1 of a row are PADDING that
   * the library may overwrite with unspecified finite-or-not values (the 8-wave kernels store whole 32-column groups when
   * N % 4 == 0 and ldc >= roundup32(N)); a caller that later reduces over the pitch instead of over N must zero the pad itself
   * (as ea_rnnt_grad does for the joint's gradient). */
  long lda, ldb, ldc, ldc2, ldr, ldaux;
  long sA_hi, sA_lo, sB_hi, sB_lo, sC_hi, sC_lo, sR_hi, sR_lo, sX_hi, sX_lo;
  float alpha, out_scale;
  /* dropout: element dropped when hash(seed, z*M*N + m*N + n) < drop_thr; kept * drop_scale */
  uint64_t drop_seed;
  uint32_t drop_thr;
  float drop_scale;
  /* split-K: the k range is cut into `splitk` chunks reduced by different workgroups; the fp32 partial
   * slabs go to `workspace` (ea_gemm_splitk_workspace_bytes) and a second kernel sums them into C
   * (honouring `accumulate`).  Requires c_f32 and no other epilogue.  kchunk is filled in by the library. */
  int splitk, kchunk;
  void* workspace;
  /* Relative-position query preparation fused into the QKV projection (fairseq/modules/multihead_attention.py:679-688:
   * q_with_bias_u = q + pos_bias_u, q_with_bias_v = q + pos_bias_v, later scaled by head_dim ** -0.5).  When q_u != NULL,
   * columns n < qsplit_n of the product are NOT written to C; the rounded bf16 value q = bf16(alpha * acc + bias[n]) is formed
   * as usual and  q_u[m][n] = bf16((q + pos_u[n]) * qscale),  q_v[m][n] = bf16((q + pos_v[n]) * qscale)  go to two bf16
   * [M][ld_q] buffers instead (pos_u / pos_v NULL: zeros; q_v NULL: q_u only) — exactly ea_relpos_q_prep applied to those
   * columns.  Requires qsplit_n % 128 == 0, N % 8 == 0, batch == 1, no split-K; the other columns take the normal epilogue. */
  void* q_u;
  void* q_v;
  const float* pos_u;
  const float* pos_v;
  long ld_q;
  int qsplit_n;
  float qscale;
} EaGemmParams;

int ea_gemm_bf16(const EaGemmParams* p, ea_stream_t stream);
long ea_gemm_splitk_workspace_bytes(int M, int N, int batch, int splitk);
/* tuning hook: 0 = automatic tile height (64-row tiles when 128x128 tiles under-fill the chip), 1 = always 128,
 * 2 = always 64; returns the previous value. */
int ea_set_gemm_variant(int v);
/* live profiling of ea_gemm_bf16 for roofline reports: enable(1) clears and starts recording one HIP-event
 * pair per launch on the launch stream; read() synchronises and returns launches, summed ms and flops. */
/* tuning hook: XCD-aware workgroup -> tile mapping; mask bit 0 = direct-to-LDS kernel, bit 1 = register-staged kernel (both
 * additionally gated on the grid shape); returns the previous mask */
int ea_set_gemm_xcd_swizzle(int mask);
/* tuning hook: direct-to-LDS ring kernel for launches whose operands are both k-contiguous (0 = off, 1 = automatic ring depth, 2..4 = forced number of stages); returns the previous value */
int ea_set_gemm_glds(int stages);
/* bf16 GEMM outputs of at least `bytes` are written with non-temporal stores (default 0 = never: measured neutral on the training step); returns the old value */
long ea_set_gemm_nt_store_min_bytes(long bytes);
/* tuning hook: 8-wavefront large-tile kernels (csrc/gemm_w8.hip) for launches with both operands k-contiguous and the lean bf16
 * epilogue: 0 = never, 1 = automatic (default: a 256 x 256 or 128 x 128 tile per CU when that grid fills the chip), 2..6 = forced
 * tile configuration (diagnostic); returns the previous value */
int ea_set_gemm_w8(int mode);
int ea_gemm_profile_enable(int on);
long ea_gemm_profile_read(double* total_ms, double* total_flops);
/* algorithmic HBM bytes of the recorded launches (operands read once, outputs written once) */
int ea_gemm_profile_bytes(double* total_bytes);
/* writes one line per recorded launch ("M N K batch a_ks b_ks splitk bm64 epilogue-bits ms"); returns the count or -1 */
long ea_gemm_profile_dump(const char* path);

/* Grouped weight-gradient GEMM: ONE launch computes, for every problem i,
 *   dW_i[n][k] += sum_m dy_i[m][n] * x_i[m][k]      (fp32, leading dim ldw)
 *   db_i[n]    += sum_m dy_i[m][n]                  (when dbias != NULL)
 * i.e. torch.nn.Linear's weight / bias gradients (torch autograd of F.linear as called by
 * fairseq/modules/conformer_layer.py:134-146, multihead_attention.py:650-688, the pointwise convolutions :79-101) for all the
 * Linear layers of one encoder layer at once: no split-K slabs, no reduce pass, no separate column-sum launches. */
#define EA_WGRAD_MAX 16
typedef struct EaWgradProblem {
  const void* dy; /* bf16 [M][ld_dy], columns 0..N-1 */
  const void* x;  /* bf16 [M][ld_x], columns 0..K-1 */
  float* dW;      /* fp32 [N][ldw] */
  float* dbias;   /* fp32 [N] or NULL */
  int M, N, K;
  long ld_dy, ld_x, ldw;
} EaWgradProblem;
typedef struct EaWgradGroup {
  int count;
  EaWgradProblem p[EA_WGRAD_MAX];
} EaWgradGroup;
int ea_wgrad_group(const EaWgradGroup* group, ea_stream_t stream);
/* tuning hook: 1 (default) = groups whose operand rows are 16-byte aligned and cover whole tiles (ld_dy >= N rounded up to the
 * tile height, ld_x >= K rounded up to 128) take the direct-to-LDS kernel with transposing fragment reads, 0 = always the
 * register-staged kernel; returns the previous value */
int ea_set_wgrad_transposing_reads(int on);
/* tuning hook for the 8-wavefront 256 x 256 kernel (csrc/wgrad_w8.hip: groups of long reductions whose 256 x 256 tile grid fills
 * the chip — the transducer joint's output layer cut into row slabs): 0 = never, 1 (default) = automatic, 2 = every group whose
 * operands are 16-byte aligned; returns the previous value.  Results are bit-identical to the 4-wave kernels. */
int ea_set_wgrad_w8(int mode);

/* ------------------------------------------------------------------------------------------
 * LayerNorm (eps, affine) — fairseq/modules/layer_norm.py:28-33; with optional fused
 * "dropout then zero padded rows" of espresso/models/transformer/speech_transformer_encoder.py:348-357.
 * x,y,dy,dx: bf16 [M][C]; gamma,beta,mean,rstd,dgamma,dbeta: fp32.  row_zero: uint8 [M] or NULL.
 * bwd accumulates (+=) into dgamma/dbeta; dx_add (bf16 [M][C] or NULL) is added to dx. */
int ea_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                     int M, int C, float eps, const uint8_t* row_zero, uint64_t drop_seed, uint32_t drop_thr,
                     float drop_scale, ea_stream_t stream);
/* fp32 islands of the reference's autocast run (fairseq/tasks/fairseq_task.py:516: LayerNorm outputs are fp32): the same
 * LayerNorm with an fp32 OUTPUT (x stays bf16, a Linear's output), and its backward with an fp32 incoming gradient.  Used by
 * the transducer joint network, which adds and rectifies the two LayerNorm outputs in fp32
 * (espresso/models/transformer/speech_transformer_transducer_base.py:292-294). */
int ea_layernorm_fwd_f32out(const void* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                            int M, int C, float eps, const uint8_t* row_zero, uint64_t drop_seed, uint32_t drop_thr,
                            float drop_scale, ea_stream_t stream);
int ea_layernorm_bwd_f32dy(const void* x, const float* dy, const float* gamma, const float* mean, const float* rstd,
                           void* dx, float* dgamma, float* dbeta, int M, int C, const uint8_t* row_zero,
                           uint64_t drop_seed, uint32_t drop_thr, float drop_scale, const void* dx_add,
                           void* workspace, ea_stream_t stream);
/* workspace (ea_layernorm_bwd_workspace_bytes, or NULL): per-block dgamma/dbeta partial rows folded by a second small
 * kernel instead of 2*C global atomics per block. */
long ea_layernorm_bwd_workspace_bytes(int M, int C);
int ea_layernorm_bwd(const void* x, const void* dy, const float* gamma, const float* mean, const float* rstd,
                     void* dx, float* dgamma, float* dbeta, int M, int C, const uint8_t* row_zero,
                     uint64_t drop_seed, uint32_t drop_thr, float drop_scale, const void* dx_add,
                     void* workspace, ea_stream_t stream);
/* the two passes of ea_layernorm_bwd separately (workspace required): the parameter-gradient reduce only feeds the optimizer,
 * so a runtime can put it on another stream */
int ea_layernorm_bwd_dx(const void* x, const void* dy, const float* gamma, const float* mean, const float* rstd, void* dx,
                        float* dgamma, float* dbeta, int M, int C, const uint8_t* row_zero, uint64_t drop_seed,
                        uint32_t drop_thr, float drop_scale, const void* dx_add, void* workspace, ea_stream_t stream);
int ea_layernorm_param_reduce(const void* workspace, float* dgamma, float* dbeta, int M, int C, ea_stream_t stream);
/* the same for up to EA_LNRED_MAX LayerNorms in one launch (all LayerNorms of one encoder layer's backward) */
#define EA_LNRED_MAX 8
typedef struct EaLnReduceItem { const void* workspace; float* dgamma; float* dbeta; int M, C; } EaLnReduceItem;
typedef struct EaLnReduceGroup { int count; EaLnReduceItem item[EA_LNRED_MAX]; } EaLnReduceGroup;
int ea_layernorm_param_reduce_group(const EaLnReduceGroup* group, ea_stream_t stream);
/* ea_layernorm_bwd_dx plus a second output out2[i] = a2 * dropout(dx[i]) with its own (seed2, thr2, scale2) mask — exactly
 * ea_scale_dropout_bf16(dx, NULL, out2, M*C, a2, 0, seed2, thr2, scale2) without the extra pass (the next residual block of
 * the backward starts with that product: FairseqDropout backward + the 0.5 FFN scale) */
int ea_layernorm_bwd_dx2(const void* x, const void* dy, const float* gamma, const float* mean, const float* rstd, void* dx,
                         float* dgamma, float* dbeta, int M, int C, const void* dx_add, void* workspace, void* out2, float a2,
                         uint64_t seed2, uint32_t thr2, float scale2, ea_stream_t stream);
/* Two LayerNorms back to back over the same rows, C <= 512: y1 = LN(x; g1, b1) (rounded to bf16: a Conformer layer's output,
 * espresso/modules/conformer_with_relative_positional_embedding_encoder_layer.py:143) and y2 = LN(y1; g2, b2) (the NEXT layer's
 * first operation, fairseq/modules/conformer_layer.py:141) in one launch — same results as two ea_layernorm_fwd calls. */
int ea_layernorm_fwd2(const void* x, const float* g1, const float* b1, void* y1, float* mean1, float* rstd1, const float* g2,
                      const float* b2, void* y2, float* mean2, float* rstd2, int M, int C, float eps, ea_stream_t stream);
/* Backward of that pair in one pass: d = bf16(LNbwd(x1, dy1; gamma1, mean1, rstd1) + dx_add), dx = bf16(LNbwd(x2, d; gamma2, mean2,
 * rstd2)), out2 = a2 * dropout(dx) (NULL: skipped) — the same values as ea_layernorm_bwd_dx followed by ea_layernorm_bwd_dx2, without
 * writing d.  ws1 / ws2 (ea_layernorm_bwd_workspace_bytes each) receive the dgamma / dbeta partials of norm 1 (the later one in the
 * forward) and norm 2: fold them with ea_layernorm_param_reduce. */
int ea_layernorm_bwd2_dx(const void* x1, const void* dy1, const float* gamma1, const float* mean1, const float* rstd1,
                         const void* dx_add, void* ws1, const void* x2, const float* gamma2, const float* mean2, const float* rstd2,
                         void* ws2, void* dx, int M, int C, void* out2, float a2, uint64_t seed2, uint32_t thr2, float scale2,
                         ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Streaming helpers (AMP weight cast fairseq/tasks/fairseq_task.py:516; FairseqDropout backward
 * fairseq/modules/fairseq_dropout.py:23-25; nn.Linear bias gradient). */
int ea_cast_f32_to_bf16(const float* src, void* dst, long n, ea_stream_t stream);
/* n <= 8 bf16 matrices in one launch: dst[i][c][r] = src[i][r][c] (rows[i] x cols[i], dense).  Used for the k-contiguous
 * copies of the Linear weights that the backward data-gradient GEMMs read (nn.Linear backward, x_grad = y_grad @ W). */
int ea_transpose_bf16_batch(const void* const* src, void* const* dst, const int* rows, const int* cols, int n, ea_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Waveform ingestion (host code: no device work, no stream) for the `wave` entries of the data json —
 * fairseq/data/audio/audio_utils.py:74-118 get_waveform (soundfile: PCM WAV and FLAC, mono = channel 0 as
 * espresso/tools/utils.py:438-440, normalization=False -> int16 scale) called per utterance by
 * espresso/data/feat_text_dataset.py:128-155 from `dataset.num_workers` DataLoader worker processes.  Files are decoded to int16
 * straight into the caller's (pinned) staging buffer; the batch call decodes many files on `num_threads` host threads without
 * touching Python objects.  Error codes: -1 unreadable, -3 not a WAV / FLAC file, -4 unsupported sample format, -5 capacity too
 * small, -6 malformed FLAC stream, -7 FLAC frame checksum mismatch. */
int ea_audio_probe(const char* path, long* num_samples, int* sample_rate, int* channels, int* bits);
long ea_audio_read_i16(const char* path, int16_t* dst, long capacity, int* sample_rate);
/* 1: the MD5 of the decoded audio equals the signature in the FLAC STREAMINFO block (or none is recorded; WAV: always 1), 0: differs */
int ea_audio_verify(const char* path);
/* file i -> dst[offsets[i] .. offsets[i+1]); lengths[i] = samples decoded (or the file's negative error); returns the failures */
int ea_audio_read_batch_i16(const char* const* paths, int n, int16_t* dst, const long* offsets, int num_threads, long* lengths,
                            int* sample_rates);

/* fp32 [M][ld_src] -> bf16 [M][ld_dst], N valid columns per row, columns N .. ld_dst-1 zero-filled (M <= 65535): the fp32
 * gradient of the vocabulary logits re-pitched for the bf16 weight / data gradient GEMMs of the output layer
 * (espresso/models/transformer/speech_transformer_encoder_model.py:207-208 fc_out, torch autograd of F.linear). */
int ea_cast_f32_to_bf16_rows(const float* src, long ld_src, void* dst, long ld_dst, long M, int N, ea_stream_t stream);
int ea_cast_bf16_to_f32(const void* src, float* dst, long n, ea_stream_t stream);
/* Per-step bookkeeping of the training step, one launch each instead of a handful of framework element-wise launches.
 * ea_subsample_lengths: src_len int64 [B] -> x_len int64 [B] = floor((src_len + total - 1) / total) (the sub-sampler's output
 *   lengths, total = product of its time strides), key_len int32 [B] the same numbers, pad_mask [B][Tp] and row_zero [B*Tp]
 *   one byte each = (t >= x_len[b]).
 * ea_stats_add4: stats[0] += a0, stats[1] += loss[0] (device scalar), stats[2] += a2, stats[3] += a3 (fp32).
 * ea_transpose_pad_bf16: dst[c][r] = src[r][c] for r < rows and 0 for rows <= r < ld_dst (src dense [rows][cols], dst
 *   [cols][ld_dst]): the k-contiguous copy of the output projection's weight with the reduction axis padded with zeros.
 * ea_permute_k_bf16: dst[n][f*C + c] = src[n][c*F + f] and, when dst_t is not NULL, dst_t[f*C + c][n] the same (the k-contiguous
 *   operand of the data gradient); ea_unpermute_k_add_f32: dst[n][c*F + f] += src[n][f*C + c] (the input
 *   axis of fc0 between the reference's channel-major order and the channels-last sub-sampler's, and its gradient back). */
int ea_subsample_lengths(const long* src_len, long* x_len, int* key_len, void* pad_mask, void* row_zero, int B, int Tp, int total,
                         ea_stream_t stream);
int ea_stats_add4(float* stats, float a0, const float* loss, float a2, float a3, ea_stream_t stream);
int ea_transpose_pad_bf16(const void* src, void* dst, int rows, int cols, long ld_dst, ea_stream_t stream);
int ea_permute_k_bf16(const void* src, void* dst, void* dst_t, int N, int C, int F, ea_stream_t stream);
int ea_unpermute_k_add_f32(const float* src, float* dst, int N, int C, int F, ea_stream_t stream);
/* out = a*x*keep(idx) + b*y  (bf16; y may be NULL: read as +0, which decides the sign of a zero result) */
int ea_scale_dropout_bf16(const void* x, const void* y, void* out, long n, float a, float b, uint64_t seed,
                          uint32_t thr, float inv_keep, ea_stream_t stream);
/* out[n] += sum_m X[m*ld+n]  (X bf16, out fp32) */
int ea_colsum_bf16(const void* X, float* out, int M, int N, long ld, ea_stream_t stream);
/* Token + positional embedding of the decoder — fairseq/models/transformer/transformer_decoder.py:296-330
 * (embed_scale * embed_tokens(prev_output_tokens) + embed_positions); bwd accumulates into dW (pad row skipped). */
int ea_embedding_fwd(const int* tokens, const int* positions, const float* W, const float* pos_table, void* out, int M,
                     int C, float scale, ea_stream_t stream);
int ea_embedding_bwd(const int* tokens, const void* dy, float* dW, int M, int C, float scale, int pad_idx,
                     ea_stream_t stream);
int ea_zero_rows_bf16(void* x, const uint8_t* row_zero, int M, int C, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused attention (flash_attention.hip): scores + rel-pos skew + key-padding / causal mask + fp32 online softmax +
 * attention dropout + P.V in one kernel; replaces the bmm / as_strided / softmax / dropout / bmm sequence of
 * fairseq/modules/multihead_attention.py:788-907 without materialising the (B*H, T, S) tensors.
 *   qu, qv : bf16 [B*T][ldq], (q + pos_bias_u) * scaling and (q + pos_bias_v) * scaling (ea_relpos_q_prep); qv = NULL
 *            selects plain attention (absolute positions, decoder self-attention, cross-attention).
 *   k, v   : bf16, row (b*S + j) * ldkv, head h at column h*dh of the given base pointers
 *   pp     : bf16 [2T-1][ldpp] projected sinusoidal table (row r <-> relative position, used column r = T-1-i+j)
 *   key_len: int [B] valid keys per sentence or NULL; causal: mask j > i + (S - T)
 *   out    : bf16 [B*T][ldo] (head h at column h*dh); lse: fp32 [H*B][T] row logsumexp (NULL to skip)
 * dropout index of element (z = h*B + b, i, j) is (z*T + i)*S + j, identical to ea_relpos_softmax_fwd.
 * ea_flash_attention_supported: dh == 64 (and T == S for rel-pos); other shapes use the unfused kernels. */
int ea_flash_attention_supported(int dh, int T, int S, int relpos);
int ea_flash_attention_fwd(const void* qu, const void* qv, long ldq, const void* k, const void* v, long ldkv,
                           const void* pp, long ldpp, const int* key_len, void* out, long ldo, float* lse, int H, int B,
                           int T, int S, int dh, int causal, uint64_t drop_seed, uint32_t drop_thr, float drop_scale,
                           void* keep_bits, ea_stream_t stream);
/* Attention-dropout keep decisions as bits (flash_relpos.hip): the rel-pos encoder kernels (qv != NULL, T == S, no causal
 * mask) read 16 keep bits per lane and key tile instead of hashing every element in each of the three kernels.  The
 * decisions are the same ea_keep(seed, (z*T + i)*S + j) as everywhere else.  keep_bits: ea_flash_keep_bits_bytes(H, B, T)
 * bytes of device memory; ea_flash_attention_fwd fills it (or expects it filled by ea_flash_keep_bits when bit 2 of
 * `causal` is set) and ea_flash_attention_bwd reads it.  keep_bits == NULL with dropout on selects the general kernels. */
long ea_flash_keep_bits_bytes(int H, int B, int T);
/* 0: the general kernels also serve the rel-pos encoder attention (A/B measurements, tests); returns the previous value */
int ea_set_flash_relpos(int on);
int ea_flash_keep_bits(void* keep_bits, int H, int B, int T, uint64_t drop_seed, uint32_t drop_thr, ea_stream_t stream);
/* Backward of ea_flash_attention_fwd (probabilities recomputed from lse; same dropout stream).
 *   out, dout : bf16 [B*T][ldo] forward output and its gradient;  D: fp32 [H*B][T] scratch (row dot dO.O)
 *   t1, t2    : bf16 [B*T][ldt], scaling * dL/dqu and scaling * dL/dqv, i.e. the gradients w.r.t. (q + pos_bias_u) and
 *               (q + pos_bias_v) before scaling (t2 / dBD / pp unused when qv == NULL)
 *   dBD       : bf16 [H*B][T][ld_bd] gradient of the raw positional logits (un-skewed, zero outside the band), the
 *               operand of the pos_proj weight gradient dpp[r] = sum_{b,i} dBD[.,i,r] qv[b,i]
 *   dk, dv    : bf16, row (b*S + j) * lddkv, head h at column h*dh (e.g. the k / v thirds of a packed dqkv buffer)  * ea_flash_attention_bwd `causal`: bit 0 = causal mask; bit 1 = the caller guarantees that the part of every dBD row outside
 * the band [T-1-i, T-1-i+S) is already zero (e.g. the same buffer was filled by a previous call with the same H, B, T, S and not
 * touched since), so the kernel only writes the band.
 *   dq        : optional (NULL, or bf16 [B*T][lddq], head h at column h*dh; qv != NULL only): t1 + t2 with the sum formed in
 *               fp32 — the gradient of the query projection's output, e.g. the q third of a packed dqkv buffer (without the
 *               positional term t1 itself is that gradient) */
int ea_flash_attention_bwd(const void* qu, const void* qv, long ldq, const void* k, const void* v, long ldkv,
                           const void* pp, long ldpp, const int* key_len, const void* out, const void* dout, long ldo,
                           const float* lse, float* D, void* t1, void* t2, long ldt, void* dBD, int ld_bd, void* dk,
                           void* dv, long lddkv, int H, int B, int T, int S, int dh, int causal, float scaling,
                           uint64_t drop_seed, uint32_t drop_thr, float drop_scale, const void* keep_bits,
                           void* dq, long lddq, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Relative-position attention glue — fairseq/modules/multihead_attention.py:679-688 (q+u, q+v,
 * scaling), :788-831 (skew), :835-874 (masks, fp32 softmax, dropout).  Score tensors are
 * [H][B][T][ld] fp32 (ac: ld_ac, bd: ld_bd >= T+S-1); probabilities bf16 [H][B][T][ld_p].
 * bd == NULL: plain attention (decoder self/cross attention); causal != 0 adds the future mask
 * (fairseq/models/transformer/transformer_decoder.py:386-398). */
int ea_relpos_q_prep(const void* qkv, long ldq, const float* u, const float* v, void* qu, void* qv, int M,
                     int C, float scaling, ea_stream_t stream);
int ea_relpos_softmax_fwd(const float* ac, const float* bd, const int* key_len, const float* attn_mask, void* P,
                          void* Pd, int H, int B, int T, int S, int ld_ac, int ld_bd, int ld_p, int causal,
                          uint64_t drop_seed, uint32_t drop_thr, float drop_scale, ea_stream_t stream);
int ea_relpos_softmax_bwd(const void* P, const float* dPd, void* dAC, void* dBD, int H, int B, int T, int S,
                          int ld_p, int ld_dp, int ld_bd, uint64_t drop_seed, uint32_t drop_thr,
                          float drop_scale, ea_stream_t stream);
int ea_add2_strided_bf16(const void* a, long lda, const void* b, long ldb, void* out, long ldo, int M, int C,
                         ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Conformer convolution module middle — fairseq/modules/conformer_layer.py:79-101:
 * GLU -> depthwise Conv1d (k in {3,7,15,31}, pad (k-1)/2, no bias) -> BatchNorm1d -> SiLU; a causal variant (left pad k-1)
 * follows the symmetric entry points, and csrc/stream_convmodule.hip streams it chunk by chunk.
 * Y: bf16 [B*T][2C] (pointwise_conv1 output); U,Z,H: bf16 [B*T][C]; w: fp32 [C][KW];
 * stats: fp64 [2][C] (sum, sum of squares) zeroed by the caller — double accumulators make the atomics' order invisible
 * in the fp32 statistics (reproducible forward); red: fp32 [2][C] zeroed by the caller; mean_rstd: fp32 [2][C].
 * ea_bn_act_* are also used for BatchNorm2d+ReLU of the sub-sampler (act = EA_ACT_RELU). */
int ea_glu_dwconv_fwd(const void* Y, const float* w, void* U, void* Z, double* stats, int B, int T, int C, int KW,
                      ea_stream_t stream);
int ea_bn_finalize(const double* stats, float* mean_rstd, float* running_mean, float* running_var, int C, float n,
                   float eps, float momentum, ea_stream_t stream);
int ea_bn_from_running(const float* running_mean, const float* running_var, float* mean_rstd, int C, float eps,
                       ea_stream_t stream);
int ea_bn_act_fwd(const void* Z, const float* mean_rstd, const float* gamma, const float* beta, void* H, long M,
                  int C, int act, ea_stream_t stream);
int ea_bn_act_bwd(const void* Z, const void* dH, const float* mean_rstd, const float* gamma, const float* beta,
                  float* red, void* dZ, float* dgamma, float* dbeta, long M, int C, int act, int training,
                  ea_stream_t stream);
/* dw += ... ; wgrad_ws: ea_dwconv_wgrad_workspace_bytes(B,T,C,KW) bytes of scratch (per-block partial slabs) */
long ea_dwconv_wgrad_workspace_bytes(int B, int T, int C, int KW);
int ea_glu_dwconv_bwd(const void* dZ, const void* Y, const void* U, const float* w, void* dY, float* dw,
                      void* wgrad_ws, int B, int T, int C, int KW, ea_stream_t stream);
/* ea_glu_dwconv_bwd with dw == NULL computes dY only; the depthwise weight gradient (optimizer-only) on its own: */
int ea_dwconv_bwd_weight(const void* dZ, const void* U, float* dw, void* wgrad_ws, int B, int T, int C, int KW, ea_stream_t stream);
/* The CAUSAL depthwise convolution (encoder.depthwise_conv_causal; the reference has no such option): left padding KW-1 and no
 * look-ahead, Z[t] = sum_k w[k] * U[t - (KW-1) + k] per utterance with zeros before frame 0, where the symmetric entry points
 * above read U[t - (KW-1)/2 + k].  Same arguments, layouts, tap order, fp32 accumulation and bf16 rounding points as their
 * twins (the same kernel templates with another left pad); ea_dwconv_wgrad_workspace_bytes serves both. */
int ea_glu_dwconv_causal_fwd(const void* Y, const float* w, void* U, void* Z, double* stats, int B, int T, int C, int KW,
                             ea_stream_t stream);
int ea_glu_dwconv_causal_bwd(const void* dZ, const void* Y, const void* U, const float* w, void* dY, float* dw,
                             void* wgrad_ws, int B, int T, int C, int KW, ea_stream_t stream);
int ea_dwconv_causal_bwd_weight(const void* dZ, const void* U, float* dw, void* wgrad_ws, int B, int T, int C, int KW,
                                ea_stream_t stream);
/* Training-mode BatchNorm + activation forward in one launch (ea_bn_finalize + ea_bn_act_fwd): mean / rstd come straight from
 * the fp64 batch sums `stats` ([2][C]: sum, sum of squares over n rows), are recorded in mean_rstd for the backward pass, the
 * running statistics are updated (torch.nn.BatchNorm1d: momentum, unbiased variance), and zero_next (fp64 [zero_n] or NULL) is
 * cleared — the statistics buffer of the next call, so that no fill launch precedes the kernel that accumulates into it. */
int ea_bn_act_fwd_train(const void* Z, const double* stats, float* mean_rstd, float* running_mean, float* running_var,
                        const float* gamma, const float* beta, void* H, long M, int C, int act, float n, float eps,
                        float momentum, double* zero_next, int zero_n, ea_stream_t stream);
/* ea_bn_act_bwd with the parameter gradients added by the apply kernel itself (no third launch) and zero_next (fp32 [zero_n]
 * or NULL) cleared for the next call's `red`. */
int ea_bn_act_bwd_fused(const void* Z, const void* dH, const float* mean_rstd, const float* gamma, const float* beta,
                        float* red, void* dZ, float* dgamma, float* dbeta, long M, int C, int act, int training,
                        float* zero_next, int zero_n, ea_stream_t stream);
/* ea_bn_act_bwd with dgamma == dbeta == NULL skips the parameter gradients; they are then taken from `red` by: */
int ea_bn_param_grad(const float* red, float* dgamma, float* dbeta, int C, ea_stream_t stream);
/* First sub-sampler layer (espresso/modules/speech_convolutions.py:78-102, layer 0): BatchNorm (+ activation) backward and the
 * 3x3 / 1-input-channel convolution's weight + bias gradient in one pass over Z and dH — dZ is formed in registers, never stored
 * (the first layer needs no data gradient).  X fp32 [B][T][F] (the feature matrix), Z / dH bf16 [B][To][Fo][CO], CO % 64 == 0;
 * red fp32 [2 CO] zeroed by the caller (receives BatchNorm's sums); dW fp32 [CO][3][3] and dbias fp32 [CO] (may be NULL)
 * accumulated; dgamma / dbeta accumulated when non-NULL. */
int ea_conv1_bn_bwd(const float* X, const void* Z, const void* dH, const float* mean_rstd, const float* gamma, const float* beta,
                    float* red, float* dgamma, float* dbeta, float* dW, float* dbias, int B, int T, int F, int CO, int sy, int sx,
                    int act, int training, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Conv2d sub-sampler — espresso/modules/speech_convolutions.py:78-102.  Channels-last bf16
 * activations [B][T][F][C]; first conv (C_in=1) direct from fp32 features [B][T][F]; later convs
 * via im2col (k = (ky*3+kx)*C + c) + ea_gemm_bf16.  Output sizes: To=(T-1)/sy+1, Fo=(F-1)/sx+1. */
int ea_conv1_fwd(const float* X, const float* W, const float* bias, void* Z, double* stats, int B, int T, int F,
                 int CO, int sy, int sx, ea_stream_t stream);
int ea_conv1_wgrad(const float* X, const void* dZ, float* dW, float* dbias, int B, int T, int F, int CO, int sy,
                   int sx, ea_stream_t stream);
/* Implicit-GEMM 3x3 convolutions (csrc/conv_igemm.hip; espresso/modules/speech_convolutions.py:78-102 and its autograd), channels-last
 * bf16 [B][T][F][C], padding 1, strides 1 or 2, Cin a multiple of 64, Cout 64 or 128 — no im2col / col2im buffers.
 *   fwd:   Z[B][To][Fo][Cout] = conv(X; W[Cout][3][3][Cin]) + bias ; stats (optional, fp64 [2*Cout], accumulated) receives the
 *          per-channel sum / sum of squares of the bf16 outputs (BatchNorm batch statistics)
 *   dgrad: dX[B][T][F][Cin] from dZ[B][To][Fo][Cout] and Wd[Cin][3][3][Cout] (the forward weight with its channel axes swapped)
 *   wgrad: dW[Cout][3][3][Cin] (fp32, +=) and dbias[Cout] (fp32, += ; may be NULL) from X and dZ; workspace from
 *          ea_conv3x3_wgrad_workspace_bytes */
int ea_conv3x3_fwd(const void* X, const void* W, const float* bias, void* Z, double* stats, int B, int T, int F, int Cin,
                   int Cout, int sy, int sx, ea_stream_t stream);
int ea_conv3x3_dgrad(const void* dZ, const void* Wd, void* dX, int B, int T, int F, int Cin, int Cout, int sy, int sx,
                     ea_stream_t stream);
long ea_conv3x3_wgrad_workspace_bytes(int B, int T, int F, int Cin, int Cout, int sy, int sx);
int ea_conv3x3_wgrad(const void* X, const void* dZ, float* dW, void* workspace, int B, int T, int F, int Cin, int Cout, int sy,
                     int sx, ea_stream_t stream);
/* ea_conv3x3_wgrad with dW in the parameter's own layout [Cout][Cin][3][3] (torch.nn.Conv2d, +=): written straight into the
 * parameter's gradient, no permuting copy and no accumulate launch afterwards */
int ea_conv3x3_wgrad_param_layout(const void* X, const void* dZ, float* dW, void* workspace, int B, int T, int F, int Cin, int Cout,
                                  int sy, int sx, ea_stream_t stream);
int ea_im2col3x3(const void* A, void* col, int B, int T, int F, int C, int sy, int sx, ea_stream_t stream);
int ea_col2im3x3(const void* dcol, void* dA, int B, int T, int F, int C, int sy, int sx, ea_stream_t stream);
int ea_colstats_bf16(const void* X, double* stats, long M, int C, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Losses.
 * log-softmax: espresso/models/transformer/speech_transformer_encoder_model.py:141-150.
 * CTC: espresso/criterions/ctc_loss.py:59-100 (F.ctc_loss, blank=<s>, sum, zero_infinity).
 *   lprobs fp32 [B][T][V]; targets int32 [B][Lmax]; nll fp32 [B] (per-utterance -log p);
 *   ea_ctc_grad: dlogits = grad_scale * d(sum nll)/d(logits), bf16 or fp32 [B][T][ld_out], columns
 *   [V, ld_out) zeroed; workspace: ea_ctc_workspace_bytes(B,T,Lmax) bytes, kept between the two calls.
 * Label-smoothed CE: espresso/criterions/label_smoothed_cross_entropy_v2.py:94-119 (uniform).
 *   out_loss[0] += sum loss, out_loss[1] += sum nll over non-pad rows. */
int ea_log_softmax_f32(const float* in, long ld_in, float* out, long M, int V, ea_stream_t stream);
int ea_log_softmax_bf16(const void* in, long ld_in, float* out, long M, int V, ea_stream_t stream);
long ea_ctc_workspace_bytes(int B, int T, int Lmax);
int ea_ctc_loss(const float* lprobs, const int* targets, const int* in_len, const int* tgt_len, float* nll,
                void* workspace, int B, int T, int V, int Lmax, int blank, ea_stream_t stream);
/* ea_ctc_loss with a second per-utterance output (may be NULL): nll_clean[b] = 0 where nll[b] is infinite, else nll[b] — the
 * criterion's zero_infinity value; nll keeps the raw value, which ea_ctc_grad tests.
 * ea_ctc_targets: target int64 [B][L] -> tgt32 int32 [B][L] (same values) and tgt_len int32 [B] = entries that are neither pad
 * nor eos (espresso/criterions/ctc_loss.py:66-68). */
int ea_ctc_loss_clean(const float* lprobs, const int* targets, const int* in_len, const int* tgt_len, float* nll,
                      float* nll_clean, void* workspace, int B, int T, int V, int Lmax, int blank, ea_stream_t stream);
int ea_ctc_targets(const long* target, int* tgt32, int* tgt_len, int B, int L, int pad, int eos, ea_stream_t stream);
/* backward of ea_ctc_loss: reads the lattice left in `workspace`; grad_scale_dev (device fp32 scalar,
 * may be NULL) multiplies grad_scale — the autograd grad_output, without a host sync. */
int ea_ctc_grad(const float* lprobs, const void* workspace, const float* nll, const int* targets,
                const int* in_len, const int* tgt_len, void* dlogits, long ld_out, int dlogits_bf16, int B, int T,
                int V, int Lmax, int blank, float grad_scale, const float* grad_scale_dev, int zero_infinity,
                ea_stream_t stream);
/* CTC greedy decoding — espresso/tools/ctc_decoder.py:172-188 (max over V, unique_consecutive, drop blank, score =
 * sum of per-frame maxima, alignments = first frame of each emitted token).  x: fp32 or bf16 [B][T][ld] log-probs. */
int ea_ctc_greedy_decode(const void* x, long ld, int x_bf16, const int* in_len, int* best, float* bestv, int* tokens,
                         int* align, int* out_len, float* score, int B, int T, int V, int blank, int pad,
                         ea_stream_t stream);
/* CTC prefix beam search (csrc/ctc_beam.hip; Hannun et al. 2014) with optional shallow fusion of one sub-word LM — the
 * neural-LM counterpart of the reference's KenLM lexicon decoder (espresso/tools/ctc_decoder.py:55-71).  One workgroup per
 * utterance; its beam lives in `workspace` (ea_ctc_prefix_beam_workspace_bytes(B, T, beam) bytes, any contents: the
 * launch with t0 == 0 initialises it).  x: fp32 or bf16 [B][T][ld] log-probs; beam <= 64; K (candidate tokens per frame)
 * <= min(64, V - 1); V <= 65535.
 * ea_ctc_prefix_beam_step: frames [t0, t1) (frames >= in_len[b] leave utterance b unchanged).  lm_rows NULL = no LM;
 *   otherwise fp32 [B*beam][ld_lm] log P_lm(. | hypothesis of that slot), read for the candidate tokens only, and
 *   t1 == t0 + 1: for every slot the step writes lm_parent int32 [B*beam] (row of the previous frame it continues),
 *   lm_token int32 [B*beam] (the token it appended; blank where it did not) and lm_keep uint8 [B*beam] (1 = no token
 *   appended: the LM state of the parent row stays).
 * ea_ctc_prefix_beam_finish: score = log(p_blank + p_nonblank) + lm_weight * (lm + log P_lm(eos | y)) + ins_bonus * |y|;
 *   the nbest best per utterance, sorted: tokens int32 [B][nbest][T] (pad after the hypothesis), lengths int32 [B][nbest],
 *   scores fp32 [B][nbest] (natural log), nhyp int32 [B] (hypotheses returned; the rest: length 0, score -inf). */
long ea_ctc_prefix_beam_workspace_bytes(int B, int T, int beam);
int ea_ctc_prefix_beam_step(const void* x, long ld, int x_bf16, const int* in_len, void* workspace, const float* lm_rows,
                            long ld_lm, int* lm_parent, int* lm_token, void* lm_keep, int B, int T, int V, int beam, int K,
                            int blank, float lm_weight, float ins_bonus, int t0, int t1, ea_stream_t stream);
int ea_ctc_prefix_beam_finish(void* workspace, const float* lm_rows, long ld_lm, float lm_weight, float ins_bonus, int eos,
                              int B, int T, int beam, int nbest, int pad, int* tokens, int* lengths, float* scores, int* nhyp,
                              ea_stream_t stream);
/* Hotword (contextual phrase) biasing of the CTC prefix beam search (csrc/ctc_beam.hip).  A context graph is the trie of the
 * phrases with Aho-Corasick failure links (tools/context_graph.py), node 0 = root, packed as
 *   cg_nodes int32 [cg_n_nodes][4] = (first edge, end edge, fail node, bits of phi fp32),
 *   cg_edges int32 [cg_n_edges][4] = (token, child node, bits of the edge boost fp32, 0), a node's edges ascending by token,
 *   cg_root  int32 [V][2]          = (the root's child by token or -1, bits of its edge boost): the first level by direct index;
 * cg_n_edges == cg_n_nodes - 1 (< 2^31 nodes).  An empty graph (the root alone, cg_edges NULL) is legal and gives the unbiased
 * results.  Every hypothesis carries a node q and a running bias b (root, 0 for the empty prefix).  Appending token v:
 * m = q; while m is not the root and has no edge v: m = fail(m); with an edge m -v-> q': b += phi(m) + boost(q') - phi(q),
 * else q' = root, b -= phi(q).  Stays change neither.  b joins the ranking score unweighted; the finish adds b - phi(q), so
 * a final score is the unbiased score of the same token sequence plus the boosts of the phrases completed along trie edges.
 * The candidate tokens of a frame stay the K best by acoustic score.  A phrase reached only through a failure link is not
 * credited.
 * ea_ctc_prefix_beam_bias_workspace_bytes / _bias_step / _bias_finish: as the three calls above (same arguments, limits and
 *   outputs) with the graph; the workspace is that of the unbiased search followed by (q, b) per slot, and one search uses
 *   the bias calls for all of its steps and its finish.
 * ea_context_graph_score: token rows int32 [N][L] with lens int32 [N] replayed through the graph: running fp32 [N][L] (b after
 *   every token; may be NULL), final_bias fp32 [N] (b - phi(q)), q_out int32 [N].  Tokens outside [0, V) match nothing.
 *   ea_context_graph_score_host: the same on host tables and host arrays (no device needed); it also checks every table
 *   index and returns -2 for a malformed graph. */
long ea_ctc_prefix_beam_bias_workspace_bytes(int B, int T, int beam);
int ea_ctc_prefix_beam_bias_step(const void* x, long ld, int x_bf16, const int* in_len, void* workspace, const float* lm_rows,
                                 long ld_lm, int* lm_parent, int* lm_token, void* lm_keep, const int* cg_nodes,
                                 const int* cg_edges, const int* cg_root, int cg_n_nodes, int cg_n_edges, int B, int T, int V,
                                 int beam, int K, int blank, float lm_weight, float ins_bonus, int t0, int t1, ea_stream_t stream);
int ea_ctc_prefix_beam_bias_finish(void* workspace, const float* lm_rows, long ld_lm, float lm_weight, float ins_bonus, int eos,
                                   const int* cg_nodes, int cg_n_nodes, int B, int T, int beam, int nbest, int pad, int* tokens,
                                   int* lengths, float* scores, int* nhyp, ea_stream_t stream);
int ea_context_graph_score_host(const int* nodes_host, const int* edges_host, const int* root_host, int n_nodes, int n_edges,
                                int V, const int* tokens_host, const int* lens_host, int N, int L, float* running_host,
                                float* final_host, int* q_host);
int ea_context_graph_score(const int* nodes, const int* edges, const int* root, int n_nodes, int n_edges, int V,
                           const int* tokens, const int* lens, int N, int L, float* running, float* final_bias, int* q_out,
                           ea_stream_t stream);
/* The streamed CTC prefix beam search: the frames of ea_ctc_prefix_beam_step / _bias_step over streams that come and go, alone,
 * with a sub-word LM, with a context graph or with both (csrc/ctc_beam.hip; the per-frame code and the beam's load and store
 * are the offline step's: one body with an offline and a streamed wrapper, the two tested against each other, so a stream fed in
 * any pieces gives bit for bit the offline results of the whole utterance).  One family: the context-graph tables are optional
 * arguments, cg_nodes == NULL is the unbiased search, otherwise the tables are validated as in ea_ctc_prefix_beam_bias_step; one
 * search passes the same graph, or none, to all of its calls.  The search state of a stream lives in one of max_streams slots of
 * `state` (max_streams * ea_ctc_prefix_beam_stream_state_bytes(max_frames, beam) bytes, slot-major).  Per slot, int32 words:
 * words = 2 + even(3 * tsize + 7 * beam + 2 + 2 * cap) + 2 * beam with cap = 1 + max_frames * beam, tsize the smallest power of
 * two >= max(64, 2 * cap) and even() rounding up to an even count: [0] frames consumed, [1] 0, then the offline workspace of one
 * utterance of max_frames frames (hash table, beam, counters, node_par / node_tok), then q int32 [beam] and b fp32 [beam], the
 * hypotheses' states in the context graph and running biases, which every slot has room for.  ..._state_bytes returns 0 for
 * max_frames < 1 or beam outside [1, 64].  Node ids are assigned in lane order and the hash table is only a lookup, so the
 * results do not depend on max_frames, which only sizes the table.  Conventions of ea_ctc_lexicon_stream_* and
 * ea_rnnt_frame_beam_stream_*: slots / slot_idx / n_new / row_off are device int32 [n]; an entry whose slot is outside
 * [0, max_streams) is skipped; a slot may be listed once per call; no call synchronises with the host; bad arguments return -2
 * and launch nothing; n <= 0 returns 0.
 * ..._reset: the listed slots get the state before frame 0 (what the offline step with t0 == 0 writes: the empty prefix, a cleared
 *   hash; frames = 0; q = 0, b = 0).
 * ..._step: one 256-thread workgroup per entry.  Entry b searches the frames j in [j0, min(j1, n_new[b])) of its piece, rows
 *   row_off[b] + j of x (fp32 or bf16 [total_rows][ld] log-probs), under the contract of ea_ctc_prefix_beam_step, and advances
 *   its slot's frame counter by the frames searched.  It is inactive — its slot untouched, its counter not advanced — if its slot
 *   is out of range, if it has no such frame, if a row of its piece lies outside [0, total_rows), or if the piece would take the
 *   slot past max_frames (counter - j0 + n_new[b] > max_frames: the counter stands at its value before the piece plus j0).
 *   Without lm_rows the whole piece is one launch (j0 = 0, j1 >= the largest count).  With lm_rows (fp32 [n*beam][ld_lm], row
 *   b * beam + beam slot) j1 == j0 + 1 is required, the launches of a piece come in the order j0 = 0, 1, ..., and the step
 *   writes lm_parent / lm_token / lm_keep [n*beam] as the offline step does, lm_parent in rows of THIS call; an inactive entry
 *   writes parent = its own row, token = blank, keep = 1 (what the offline step writes for t >= in_len).
 * ..._finish: ea_ctc_prefix_beam_finish (with cg_nodes: _bias_finish) per listed slot into tokens int32 [n][nbest][max_u]
 *   (pad-filled; longer hypotheses are cut at max_u and their lengths clipped), lengths / scores [n][nbest], nhyp [n]; lm_rows
 *   fp32 [n*beam][ld_lm] in the order of `slots`.  The state is read only, so the call is valid mid-stream; a reset slot without
 *   frames returns the empty hypothesis, as the offline search does for T = 0.
 * ..._partial: per listed slot the live hypothesis with the best in-beam score log(p_blank + p_nonblank) + lm_weight * lm +
 *   ins_bonus * |y| (+ b with biased != 0; ties: the lower beam slot) into tokens int32 [n][max_u], lengths / scores [n] (that
 *   value), and stable_len [n]: the length of the longest common prefix of the live hypotheses with a finite in-beam score (of
 *   all live ones when none is finite), the depth of their lowest common ancestor in node_par.  Every hypothesis a later finish
 *   can return with a finite score starts with those tokens.  lm_weight = 0 when no LM is fused.  The state is read only. */
long ea_ctc_prefix_beam_stream_state_bytes(int max_frames, int beam);
int ea_ctc_prefix_beam_stream_reset(void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                    ea_stream_t stream);
int ea_ctc_prefix_beam_stream_step(const void* x, long ld, int x_bf16, long total_rows, const int* slot_idx, const int* n_new,
                                   const int* row_off, int j0, int j1, int n, void* state, const float* lm_rows, long ld_lm,
                                   int* lm_parent, int* lm_token, void* lm_keep, const int* cg_nodes, const int* cg_edges,
                                   const int* cg_root, int cg_n_nodes, int cg_n_edges, int max_streams, int max_frames, int V,
                                   int beam, int K, int blank, float lm_weight, float ins_bonus, ea_stream_t stream);
int ea_ctc_prefix_beam_stream_finish(const void* state, const int* slots, int n, const float* lm_rows, long ld_lm, float lm_weight,
                                     float ins_bonus, int eos, const int* cg_nodes, int cg_n_nodes, int max_streams,
                                     int max_frames, int beam, int nbest, int pad, int max_u, int* tokens, int* lengths,
                                     float* scores, int* nhyp, ea_stream_t stream);
int ea_ctc_prefix_beam_stream_partial(const void* state, const int* slots, int n, float lm_weight, float ins_bonus, int biased,
                                      int max_streams, int max_frames, int beam, int pad, int max_u, int* tokens, int* lengths,
                                      float* scores, int* stable_len, ea_stream_t stream);
/* Time stamps for the CTC prefix beam search, offline and streamed (csrc/ctc_beam.hip, the kTimes instantiations).  Every
 * hypothesis also carries vb / vnb: pb / pnb with max in place of log-add-exp, the score of its best single alignment path (the
 * LM, insertion-bonus and bias terms depend on the tokens only and stay out), and eb / enb: pointers into a per-utterance pool of
 * time nodes (parent time node, frame), node 0 = no tokens.  Stay: vb' = max(vb, vnb) + x[blank] with the pointer of the larger
 * (tie: eb); vnb' = vnb + x[last] (-inf if last is no candidate), enb' = enb.  Extension by c: from (vb, eb) if c == last, else
 * from the larger of (vb, eb), (vnb, enb) (tie: the blank one): vnb'' = that + x[c] with a new time node (its pointer, t),
 * vb'' = -inf.  An extension merging into a stay replaces the stay's (vnb', enb') only if strictly larger.  Time nodes are made
 * for selected candidates only (<= beam per frame, numbered in lane order).  Tokens, scores, n-best order and the triples are
 * those of the search without times, bit for bit.  Each call takes the arguments of its twin (the graph tables optional as in
 * ea_ctc_prefix_beam_stream_*: cg_nodes == NULL is the unbiased search on the unbiased workspace, otherwise the workspace is the
 * bias one) plus a separate times workspace / times state; the beam workspace / stream state is the twin's, unchanged.
 * 4-byte words per utterance (T frames) or per stream slot (T = max_frames):
 *   times words = 4 * beam + 2 + 2 * cap, cap = 1 + T * beam
 * (vb, vnb fp32 [beam]; eb, enb int32 [beam]; node counter, 0; tpar int32 [cap]; tfrm int32 [cap]).  ..._bytes return 0 for
 * arguments out of range.  Bad arguments (those of the twin, a NULL times buffer or output) return -2 and launch nothing.
 * ..._times_step / _stream_times_step: as the twin; the launch with t0 == 0 also initialises the times workspace; a streamed entry
 *   that is not due leaves its slot and its times slot untouched.  Streamed frames count from the stream's first frame.
 * ..._stream_times_reset: resets the listed slots of `state` as ..._stream_reset does, and their times slots.
 * ..._times_finish / _stream_times_finish: as the twin, and times int32 [..][nbest][max_u] (offline: max_u = T): times[u] = the
 *   frame at which token u starts on the best path of the larger of (vb, vnb) (tie: eb), -1 after the hypothesis, cut at max_u
 *   as tokens is; vscores fp32 [..][nbest] = max(vb, vnb) (-inf where there is no hypothesis).  Read only: valid mid-stream. */
long ea_ctc_prefix_beam_times_workspace_bytes(int B, int T, int beam);
int ea_ctc_prefix_beam_times_step(const void* x, long ld, int x_bf16, const int* in_len, void* workspace, void* times_workspace,
                                  const float* lm_rows, long ld_lm, int* lm_parent, int* lm_token, void* lm_keep,
                                  const int* cg_nodes, const int* cg_edges, const int* cg_root, int cg_n_nodes, int cg_n_edges,
                                  int B, int T, int V, int beam, int K, int blank, float lm_weight, float ins_bonus, int t0, int t1,
                                  ea_stream_t stream);
int ea_ctc_prefix_beam_times_finish(void* workspace, const void* times_workspace, const float* lm_rows, long ld_lm, float lm_weight,
                                    float ins_bonus, int eos, const int* cg_nodes, int cg_n_nodes, int B, int T, int beam,
                                    int nbest, int pad, int* tokens, int* lengths, float* scores, int* nhyp, int* times,
                                    float* vscores, ea_stream_t stream);
long ea_ctc_prefix_beam_stream_times_state_bytes(int max_frames, int beam);
int ea_ctc_prefix_beam_stream_times_reset(void* state, void* times_state, const int* slots, int n, int max_streams, int max_frames,
                                          int beam, ea_stream_t stream);
int ea_ctc_prefix_beam_stream_times_step(const void* x, long ld, int x_bf16, long total_rows, const int* slot_idx, const int* n_new,
                                         const int* row_off, int j0, int j1, int n, void* state, void* times_state,
                                         const float* lm_rows, long ld_lm, int* lm_parent, int* lm_token, void* lm_keep,
                                         const int* cg_nodes, const int* cg_edges, const int* cg_root, int cg_n_nodes,
                                         int cg_n_edges, int max_streams, int max_frames, int V, int beam, int K, int blank,
                                         float lm_weight, float ins_bonus, ea_stream_t stream);
int ea_ctc_prefix_beam_stream_times_finish(const void* state, const void* times_state, const int* slots, int n, const float* lm_rows,
                                           long ld_lm, float lm_weight, float ins_bonus, int eos, const int* cg_nodes,
                                           int cg_n_nodes, int max_streams, int max_frames, int beam, int nbest, int pad, int max_u,
                                           int* tokens, int* lengths, float* scores, int* nhyp, int* times, float* vscores,
                                           ea_stream_t stream);
/* The endpoint probe of the streamed CTC prefix beam search with times (csrc/ctc_beam.hip): whether an utterance has ended in a
 * slot, from state the kernels above already write.  state / times_state: those of ea_ctc_prefix_beam_stream_times_* (biased != 0:
 * the searches ran with a graph); slots device int32 [n]; lm_weight / ins_bonus / biased as ea_ctc_prefix_beam_stream_partial takes
 * them.  Per listed slot, with F = its frame counter: best = the live hypothesis ..._stream_partial reports (same score, tie rule
 * and handling of non-finite scores; the empty hypothesis for F == 0 or no hypothesis), L = its length, E = the frame, counted
 * from the slot's first frame, at which its last token starts on its best path: what ..._stream_times_finish writes as
 * times[L - 1] for it (tfrm of the pointer of the larger of (vb, eb), (vnb, enb); tie: eb), -1 when L == 0.  rule = the first
 * that holds of 1 "silence": L > 0 and F - 1 - E >= silence_frames; 2 "empty": L == 0 and F >= empty_frames; 3 "length":
 * F >= segment_frames; else 0.  A threshold <= 0 switches its rule off.  out int32 [n][4] = (rule, F, L, E); a slot outside
 * [0, max_streams) writes (0, 0, 0, -1).  Both states are read only.  Bad arguments (a NULL buffer, max_streams or max_frames < 1,
 * beam outside [1, 64]) return -2 and launch nothing; n <= 0 returns 0. */
int ea_ctc_prefix_beam_stream_endpoint(const void* state, const void* times_state, const int* slots, int n, float lm_weight,
                                       float ins_bonus, int biased, int max_streams, int max_frames, int beam, int silence_frames,
                                       int empty_frames, int segment_frames, int* out, ea_stream_t stream);
/* Frame-synchronous transducer beam search (csrc/rnnt_beam.hip; at most one symbol per encoder frame and hypothesis, equal
 * token sequences merged — "modified beam search") with optional mass-preserving shallow fusion of one sub-word LM: the
 * transducer counterpart of ea_ctc_prefix_beam_*.  Hypotheses are distinct token sequences with a score (natural log), at most
 * `beam` per utterance, best first; they live in `workspace` (ea_rnnt_frame_beam_workspace_bytes(B, T, beam) bytes, any
 * contents: the step with t == 0 initialises it).  beam <= 64; K (extensions per hypothesis and frame) <= min(64, V - 1);
 * V <= 65535; bad arguments return -2 and launch nothing.
 * ea_rnnt_frame_beam_step: frame t (0 <= t < T; frames >= in_len[b] leave utterance b unchanged).  logits: the joint's fp32
 *   logits of THIS frame, [B*beam][ld], row b * beam + slot — the step never sees the encoder, so the state between two calls
 *   is exactly the workspace (a streamed search can feed it frame by frame).  Rows of dead slots (slot >= number of
 *   hypotheses) are not read.  Per live row: r = log_softmax(logits[:V] / temperature); with lm_rows (fp32 [B*beam][ld_lm],
 *   log P_lm(. | hypothesis of that slot), finite entries; NULL or lm_weight == 0 = no LM, the rows are not read)
 *   f_v = r_v + lm_weight * lm_v for v != blank, renormalised so that the
 *   non-blank mass of r is kept, r_blank untouched (lm_no_blank != 0: the LM has V - 1 entries and token v > blank reads
 *   column v - 1); with eos >= 0 (-1 = none) r_blank = logaddexp(r_blank, r_eos) and r_eos = -inf.  Candidates: the stay
 *   (score + r_blank) and the extensions by the K non-blank tokens with the largest finite r_v (ties: lower id); an extension
 *   equal to a hypothesis of the beam merges into that hypothesis' stay (log-add-exp); the `beam` best finite candidates
 *   survive (ties: parent slot, stay before extension, token id).  For every slot the step writes parent int32 [B*beam] (row
 *   of the previous frame it continues), token int32 [B*beam] (the token it appended; blank for a stay) and keep uint8
 *   [B*beam] (1 = stay: the predictor / LM state of the parent row stands).
 * ea_rnnt_frame_beam_finish: final score = the score, or with normalize != 0 score / max(1, length); the nbest best per
 *   utterance, sorted (ties: slot); outputs as ea_ctc_prefix_beam_finish. */
long ea_rnnt_frame_beam_workspace_bytes(int B, int T, int beam);
int ea_rnnt_frame_beam_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank, const int* in_len,
                            void* workspace, int* parent, int* token, void* keep, int B, int T, int V, int beam, int K, int blank,
                            int eos, float temperature, float lm_weight, int t, ea_stream_t stream);
int ea_rnnt_frame_beam_finish(void* workspace, int B, int T, int beam, int nbest, int pad, int normalize, int* tokens,
                              int* lengths, float* scores, int* nhyp, ea_stream_t stream);
/* The streamed frame-synchronous transducer beam search: the same frames, one per call, over streams that come and go
 * (csrc/rnnt_beam.hip; the per-frame code is the offline step's: one body with an offline and a streamed wrapper, the two
 * tested against each other, so a stream fed in any pieces gives bit for bit the offline results of the whole utterance,
 * whatever max_frames >= its length).  The search state of a stream lives in one of max_streams
 * slots of `state` (max_streams * ea_rnnt_frame_beam_stream_state_bytes(max_frames, beam) bytes, slot-major).  Per slot, int32
 * words: words = 2 + even(3 * tsize + 5 * beam + 2 + 2 * cap + 2 * beam + 2 * beam * 64) with cap = 1 + max_frames * beam, tsize
 * the smallest power of two >= max(64, 2 * cap) and even() rounding up to an even count: [0] frames consumed, [1] 0, then the
 * offline workspace of one utterance of max_frames frames — hash table, beam, counters, node_par / node_tok and the
 * row-to-select hand-over (rblank, rnc, ctok, cval), which lives in the slot, not in a per-call scratch.  ..._state_bytes
 * returns 0 for max_frames < 1 or beam outside [1, 64].  Conventions of ea_stream_attention / ea_ctc_lexicon_stream_*: slots /
 * slot_idx / n_new are device int32 [n]; an entry whose slot is outside [0, max_streams) is skipped; no call synchronises with
 * the host; bad arguments return -2 and launch nothing; n <= 0 returns 0.
 * ..._reset: the listed slots get the state before frame 0 (the empty hypothesis with score 0, a cleared hash, frames = 0).
 * ..._step: ONE encoder frame for each of the n listed streams: logits fp32 [n*beam][ld], row b * beam + beam slot (lm_rows
 *   likewise), the j-th new frame of this round.  Entry b is active iff its slot is in range, j < n_new[b] and the slot has
 *   consumed fewer than max_frames frames; an active entry does one frame of the contract of ea_rnnt_frame_beam_step and
 *   increments the slot's frame counter; an inactive one leaves its slot untouched and writes parent = identity, token =
 *   blank, keep = 1 (what the offline step writes for t >= in_len).  parent / token / keep are [n*beam], parent in rows of
 *   THIS call (b * beam + slot of the previous frame).  Rows of dead beam slots are not read.  A slot may be listed once.
 * ..._finish: ea_rnnt_frame_beam_finish per listed slot into tokens int32 [n][nbest][max_u] (pad-filled; longer hypotheses
 *   are cut at max_u), lengths / scores [n][nbest], nhyp [n]; the state is read only, so the call is valid mid-stream.
 * ..._partial: per listed slot the live hypothesis with the best score s (the quantity the search prunes by; ties: the lower
 *   beam slot) into tokens int32 [n][max_u], lengths / scores [n], and stable_len [n]: the length of the longest common prefix
 *   of all live hypotheses (the depth of their lowest common ancestor in the prefix table).  Every hypothesis a later finish
 *   can return starts with those tokens.  The state is read only. */
long ea_rnnt_frame_beam_stream_state_bytes(int max_frames, int beam);
int ea_rnnt_frame_beam_stream_reset(void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                    ea_stream_t stream);
int ea_rnnt_frame_beam_stream_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank,
                                   const int* slot_idx, const int* n_new, int j, int n, void* state, int* parent, int* token,
                                   void* keep, int max_streams, int max_frames, int V, int beam, int K, int blank, int eos,
                                   float temperature, float lm_weight, ea_stream_t stream);
int ea_rnnt_frame_beam_stream_finish(const void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                     int nbest, int pad, int normalize, int max_u, int* tokens, int* lengths, float* scores,
                                     int* nhyp, ea_stream_t stream);
int ea_rnnt_frame_beam_stream_partial(const void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                      int pad, int max_u, int* tokens, int* lengths, float* scores, int* stable_len,
                                      ea_stream_t stream);
/* Hotword (contextual phrase) biasing of the frame-synchronous transducer beam search, offline and streamed
 * (csrc/rnnt_beam.hip, the kBias instantiations).  The context graph, its packed tables (cg_nodes, cg_edges, cg_root with
 * cg_n_edges == cg_n_nodes - 1; an empty graph = the root alone, cg_edges NULL, is legal and gives the unbiased results bit for
 * bit) and the automaton step are those of ea_ctc_prefix_beam_bias_* above; the beam is that of ea_rnnt_frame_beam_step.  Every
 * hypothesis carries (q, b), (root, 0) for the empty one; the unbiased score s is kept as it is.  The row phase is unchanged:
 * the K candidate tokens of a row stay the K with the largest fused r_v, so biasing re-ranks and does not bring a token back,
 * and with it K = beam is no longer a global top-`beam`.  An extension takes one automaton step from its parent's (q, b); a stay
 * changes neither; a merge is decided as before and adds the scores s only — (q, b) are functions of the token sequence, so
 * the merged hypothesis keeps the stay's.  A candidate is live iff its s is finite; the `beam` best by (-(s + b'), key) survive,
 * keys and triples as before.  Finish: s + b - phi(q), with normalize != 0 divided by max(1, length): the unbiased final of the
 * same tokens plus the boosts of the phrases completed along trie edges, before the division.  A phrase reached only through a
 * failure link is not credited; phrases of at most 64 tokens; one graph per search.  One search uses the bias calls for all of
 * its steps, its finish and its partials.  Bad arguments (those of the unbiased twin, NULL cg_nodes / cg_root, cg_edges NULL with
 * cg_n_edges > 0, cg_n_edges != cg_n_nodes - 1) return -2 and launch nothing.
 * ea_rnnt_frame_beam_bias_workspace_bytes / _bias_step / _bias_finish: as ea_rnnt_frame_beam_workspace_bytes / _step / _finish
 *   with the graph (same arguments, limits and outputs); the workspace is that of the unbiased search followed by (q, b) per
 *   slot: 2 * beam more 4-byte words per utterance.
 * ea_rnnt_frame_beam_stream_bias_state_bytes / _bias_reset / _bias_step / _bias_finish / _bias_partial: as
 *   ea_rnnt_frame_beam_stream_state_bytes / _reset / _step / _finish / _partial with the graph.  Per slot, int32 words:
 *   bias words = words + 2 * beam = 2 + even(3 * tsize + 5 * beam + 2 + 2 * cap + 2 * beam + 2 * beam * 64) + 2 * beam (cap, tsize,
 *   even() as above): the unbiased slot followed by q int32 [beam] and b fp32 [beam].  A stream fed in any pieces gives bit for
 *   bit what the offline bias calls give for the whole utterance.  _bias_partial returns the live hypothesis with the best
 *   s + b (ties: the lower beam slot) and that value as its score; stable_len as in the unbiased call. */
long ea_rnnt_frame_beam_bias_workspace_bytes(int B, int T, int beam);
int ea_rnnt_frame_beam_bias_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank, const int* in_len,
                                 void* workspace, int* parent, int* token, void* keep, const int* cg_nodes, const int* cg_edges,
                                 const int* cg_root, int cg_n_nodes, int cg_n_edges, int B, int T, int V, int beam, int K, int blank,
                                 int eos, float temperature, float lm_weight, int t, ea_stream_t stream);
int ea_rnnt_frame_beam_bias_finish(void* workspace, const int* cg_nodes, int cg_n_nodes, int B, int T, int beam, int nbest, int pad,
                                   int normalize, int* tokens, int* lengths, float* scores, int* nhyp, ea_stream_t stream);
long ea_rnnt_frame_beam_stream_bias_state_bytes(int max_frames, int beam);
int ea_rnnt_frame_beam_stream_bias_reset(void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                         ea_stream_t stream);
int ea_rnnt_frame_beam_stream_bias_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank,
                                        const int* slot_idx, const int* n_new, int j, int n, void* state, int* parent, int* token,
                                        void* keep, const int* cg_nodes, const int* cg_edges, const int* cg_root, int cg_n_nodes,
                                        int cg_n_edges, int max_streams, int max_frames, int V, int beam, int K, int blank, int eos,
                                        float temperature, float lm_weight, ea_stream_t stream);
int ea_rnnt_frame_beam_stream_bias_finish(const void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                          const int* cg_nodes, int cg_n_nodes, int nbest, int pad, int normalize, int max_u,
                                          int* tokens, int* lengths, float* scores, int* nhyp, ea_stream_t stream);
int ea_rnnt_frame_beam_stream_bias_partial(const void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                           int pad, int max_u, int* tokens, int* lengths, float* scores, int* stable_len,
                                           ea_stream_t stream);
/* Time stamps for the frame-synchronous transducer beam search, offline and streamed (csrc/rnnt_beam.hip, the kTimes
 * instantiations).  Every hypothesis also carries v, which accumulates the same fused r as its score with max in place of
 * log-add-exp at a merge (the score of its best single alignment path), and e, a pointer into a per-utterance pool of time
 * nodes (parent time node, frame), node 0 = no tokens.  Stay: v' = v + r_blank, e' = e.  Extension by u: v'' = v + r_u with a
 * new time node (e, t).  An extension merging into a stay replaces the stay's (v', e') only if strictly larger.  Time nodes are
 * made for selected candidates only (<= beam per frame).  Tokens, scores, n-best order and the triples are those of the search
 * without times, bit for bit; the row phase is the twin's.  Each call takes the arguments of its twin with the graph tables
 * optional (cg_nodes == NULL: the unbiased search on the unbiased workspace / state; otherwise the bias workspace / state) plus
 * a separate times workspace / times state; the beam workspace / stream state is the twin's, unchanged.  4-byte words per
 * utterance (T frames) or per stream slot (T = max_frames):
 *   times words = 2 * beam + 2 + 2 * cap, cap = 1 + T * beam
 * (v fp32 [beam]; e int32 [beam]; node counter, 0; tpar int32 [cap]; tfrm int32 [cap]).  ..._bytes return 0 for arguments out of
 * range.  Bad arguments (those of the twin, a NULL times buffer or output) return -2 and launch nothing.
 * ..._times_step / _stream_times_step: as the twin; the step with t == 0 also initialises the times workspace; a streamed entry
 *   that is not active leaves its slot and its times slot untouched.  Streamed frames count from the stream's first frame.
 * ..._stream_times_reset: resets the listed slots of `state` (biased != 0: a bias state) as the twin's reset does, and their
 *   times slots.
 * ..._times_finish / _stream_times_finish: as the twin, and times int32 [..][nbest][max_u] (offline: max_u = T): times[u] = the
 *   frame at which token u is emitted on that path, -1 after the hypothesis, cut at max_u as tokens is; vscores fp32
 *   [..][nbest] = v, never normalised (-inf where there is no hypothesis).  Read only: valid mid-stream. */
long ea_rnnt_frame_beam_times_workspace_bytes(int B, int T, int beam);
int ea_rnnt_frame_beam_times_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank, const int* in_len,
                                  void* workspace, void* times_workspace, int* parent, int* token, void* keep, const int* cg_nodes,
                                  const int* cg_edges, const int* cg_root, int cg_n_nodes, int cg_n_edges, int B, int T, int V,
                                  int beam, int K, int blank, int eos, float temperature, float lm_weight, int t, ea_stream_t stream);
int ea_rnnt_frame_beam_times_finish(void* workspace, const void* times_workspace, const int* cg_nodes, int cg_n_nodes, int B, int T,
                                    int beam, int nbest, int pad, int normalize, int* tokens, int* lengths, float* scores, int* nhyp,
                                    int* times, float* vscores, ea_stream_t stream);
long ea_rnnt_frame_beam_stream_times_state_bytes(int max_frames, int beam);
int ea_rnnt_frame_beam_stream_times_reset(void* state, void* times_state, const int* slots, int n, int biased, int max_streams,
                                          int max_frames, int beam, ea_stream_t stream);
int ea_rnnt_frame_beam_stream_times_step(const float* logits, long ld, const float* lm_rows, long ld_lm, int lm_no_blank,
                                         const int* slot_idx, const int* n_new, int j, int n, void* state, void* times_state,
                                         int* parent, int* token, void* keep, const int* cg_nodes, const int* cg_edges,
                                         const int* cg_root, int cg_n_nodes, int cg_n_edges, int max_streams, int max_frames, int V,
                                         int beam, int K, int blank, int eos, float temperature, float lm_weight, ea_stream_t stream);
int ea_rnnt_frame_beam_stream_times_finish(const void* state, const void* times_state, const int* slots, int n, int max_streams,
                                           int max_frames, int beam, const int* cg_nodes, int cg_n_nodes, int nbest, int pad,
                                           int normalize, int max_u, int* tokens, int* lengths, float* scores, int* nhyp, int* times,
                                           float* vscores, ea_stream_t stream);
/* The endpoint probe of the streamed transducer beam search with times (csrc/rnnt_beam.hip): ea_ctc_prefix_beam_stream_endpoint
 * for state / times_state of ea_rnnt_frame_beam_stream_times_* (biased != 0: a bias state, as in ..._stream_times_reset).  best =
 * the live hypothesis ..._stream_partial / _bias_partial reports (score s, biased: s + b; ties: the lower beam slot), L = its
 * length, E = tfrm[e]: the frame at which its last token is emitted on its best path, what ..._stream_times_finish writes as
 * times[L - 1] for it, -1 when L == 0.  Rules, thresholds, out int32 [n][4] = (rule, F, L, E), the row of a slot out of range
 * and the refusals are those of the CTC probe.  Both states are read only. */
int ea_rnnt_frame_beam_stream_endpoint(const void* state, const void* times_state, const int* slots, int n, int biased,
                                       int max_streams, int max_frames, int beam, int silence_frames, int empty_frames,
                                       int segment_frames, int* out, ea_stream_t stream);
/* Word n-gram LM (ARPA) and lexicon-constrained CTC prefix beam search with its fusion (csrc/ctc_lexicon_beam.hip) — the
 * search the reference takes from Flashlight's KenLM lexicon decoder (espresso/tools/ctc_decoder.py:24-71).
 * ea_ngram_create: parses a plain-text ARPA file of order <= 6 at `path` into host tables and writes an opaque handle to
 *   *(void**)handle_host; 0 = success, -1 = the file cannot be read, -3 = malformed (err_host, err_cap bytes, then names the
 *   line).  Log10 values become natural logs.  Word ids are the unigrams in file order (ea_ngram_vocab: the words, each
 *   followed by '\n'; returns the bytes needed and writes them when cap suffices).  ea_ngram_info: meta_host int[4] =
 *   order, <unk>, <s>, </s> ids (-1 where absent; <s> and </s> are required), counts_host long[6] = n-grams per order.
 *   ea_ngram_records: the records of one order, in table order: ngrams_host int [count][order] word ids, logp_host and
 *   bow_host fp32 [count].  ea_ngram_upload copies the tables to the current device once (later calls return 0); the
 *   `ngram` / `handle` arguments below are such handles (not device pointers).  ea_ngram_destroy frees both copies.
 * ea_ngram_score: out fp32 [N] = ln P(words[i] | ctx[i]) with ARPA backoff; ctx int32 [N][order - 1] oldest first,
 *   front-padded with -1 (<s> is an ordinary context word); a word outside the vocabulary scores as <unk> (-inf without).
 *   ea_ngram_score_host: the same on the host tables and host arrays (no device needed).
 * ea_ctc_lexicon_beam_search: the prefix beam search of ea_ctc_prefix_beam_step (K best non-blank tokens per frame, stay and
 *   extend, merging of equal token sequences, the same tie rules) with a closed-vocabulary lexicon and n-gram fusion, the
 *   whole batch in one launch (one workgroup per utterance).  Score of a hypothesis with completed words w_1..w_m and a
 *   partial word p:  log(p_b + p_nb) + lm_weight * (L(y) + S(p)) + word_score * m + ins_bonus * |y|,  L(y) = sum of
 *   ln P(w_i | history) with <s> as the start, S(p) = the trie node's smear (max unigram ln P below it, 0 at the root); the
 *   final score completes the pending word and adds lm_weight * ln P(</s> | history).  Leaving the trie, ending a word on a
 *   node that is no word, an empty word and a pending non-word at the end score -inf.  Lexicon trie in CSR form (device,
 *   node 0 = root): children of node n are trie_tok / trie_child [trie_off[n] .. trie_off[n + 1]) with trie_tok ascending;
 *   trie_word int32 [nodes] = LM word id ending at the node or -1; trie_smear fp32 [nodes].  A word ends on token `space`
 *   (space mode, space >= 0) or, with space < 0, before every token v with word_start uint8 [V] set.  x: fp32 or bf16
 *   [B][T][ld] log-probs; beam <= 64, K <= min(64, V - 1), V <= 65535, nbest <= beam.  workspace:
 *   ea_ctc_lexicon_beam_workspace_bytes(B, T, beam) bytes, any contents.  Outputs as ea_ctc_prefix_beam_finish: tokens
 *   int32 [B][nbest][T], lengths, scores (natural log), nhyp = the number of finite hypotheses returned (0 for an empty
 *   utterance or when none is finite). */
int ea_ngram_create(const char* path, void* handle_host, char* err_host, long err_cap);
int ea_ngram_destroy(void* handle);
int ea_ngram_info(const void* handle, int* meta_host, long* counts_host);
long ea_ngram_vocab(const void* handle, char* buf_host, long cap);
long ea_ngram_records(const void* handle, int order, int* ngrams_host, float* logp_host, float* bow_host);
int ea_ngram_upload(void* handle);
int ea_ngram_score_host(const void* handle, const int* ctx_host, const int* words_host, int N, float* out_host);
int ea_ngram_score(const void* handle, const int* ctx, const int* words, int N, float* out, ea_stream_t stream);
long ea_ctc_lexicon_beam_workspace_bytes(int B, int T, int beam);
int ea_ctc_lexicon_beam_search(const void* x, long ld, int x_bf16, const int* in_len, void* workspace, const void* ngram,
                               const int* trie_off, const int* trie_tok, const int* trie_child, const int* trie_word,
                               const float* trie_smear, const void* word_start, int space, int B, int T, int V, int beam, int K,
                               int blank, float lm_weight, float word_score, float ins_bonus, int nbest, int pad, int* tokens,
                               int* lengths, float* scores, int* nhyp, ea_stream_t stream);
/* The same search, resumable per stream slot (streaming recognition): the frames of an utterance arrive in pieces, and the
 * results are those of ea_ctc_lexicon_beam_search over all of them, bit for bit — the per-frame code is the same.
 *   state   : caller-allocated device buffer [max_streams][ea_ctc_lexicon_stream_state_bytes(max_frames, beam)], 8-byte
 *             aligned.  A slot holds what the offline kernel has live between two frames: the beam (hypothesis count, and per
 *             hypothesis p_b, p_nb, LM sum, length, last token, prefix node, its parent, trie node, word context), the
 *             prefix table with its hash, sized for max_frames frames, and the number of frames consumed.  max_frames, beam
 *             and the n-gram order are fixed for the life of the buffer.
 *   slots   : int [n], device: the stream slots a call handles; entries outside [0, max_streams) are skipped.
 * ea_ctc_lexicon_stream_reset  : the given slots get the state before frame 0 (empty prefix, <s> context, cleared hash).
 *             A kernel on `stream`, no host synchronisation.  A slot must be reset before its first step.
 * ea_ctc_lexicon_stream_step   : slot_idx, n_new, row_off int [n] (device), as ea_stream_attention takes them: entry b is
 *             stream slot_idx[b] with n_new[b] new frames at rows row_off[b] .. of x, fp32 or bf16 [total_rows][ld]
 *             log-probs.  One launch, one workgroup per entry: the slot's beam is loaded into LDS, the frames are searched,
 *             the beam is stored.  n_new[b] == 0, out-of-range entries and an entry that would take its slot past max_frames
 *             leave the slot untouched.  A slot may appear once per call.  The other arguments are those of
 *             ea_ctc_lexicon_beam_search and must not change between the steps of a stream.
 * ea_ctc_lexicon_stream_finish : the finish of the offline search for the given slots (pending word, ln P(</s> | history), the
 *             nbest best finite hypotheses, sorted): tokens int32 [n][nbest][max_u] (pad after the hypothesis; tokens beyond
 *             max_u are dropped and the length is clipped: give max_u >= the frames consumed), lengths, scores [n][nbest],
 *             nhyp [n] (0 for a slot without frames).  The state is not modified: it is a readout, valid mid-stream.
 * ea_ctc_lexicon_stream_partial: per given slot, the live hypothesis with the best in-beam score
 *             log(p_b + p_nb) + lm + ins_bonus * length (the smeared LM sum the search prunes by; ties: the lower beam slot):
 *             tokens int32 [n][max_u], lengths, scores [n], and stable_len [n] = the length of the longest common prefix of
 *             the live hypotheses whose in-beam score is finite (of all live ones when none is).  Every hypothesis a later
 *             finish can return starts with those tokens.  The state is not modified. */
long ea_ctc_lexicon_stream_state_bytes(int max_frames, int beam);
int ea_ctc_lexicon_stream_reset(void* state, const int* slots, int n, const void* ngram, int max_streams, int max_frames,
                                int beam, ea_stream_t stream);
int ea_ctc_lexicon_stream_step(const void* x, long ld, int x_bf16, long total_rows, const int* slot_idx, const int* n_new,
                               const int* row_off, int n, void* state, const void* ngram, const int* trie_off,
                               const int* trie_tok, const int* trie_child, const int* trie_word, const float* trie_smear,
                               const void* word_start, int space, int max_streams, int max_frames, int V, int beam, int K,
                               int blank, float lm_weight, float word_score, float ins_bonus, ea_stream_t stream);
int ea_ctc_lexicon_stream_finish(const void* state, const int* slots, int n, const void* ngram, const int* trie_word,
                                 const float* trie_smear, int max_streams, int max_frames, int beam, float lm_weight,
                                 float word_score, float ins_bonus, int nbest, int pad, int max_u, int* tokens, int* lengths,
                                 float* scores, int* nhyp, ea_stream_t stream);
int ea_ctc_lexicon_stream_partial(const void* state, const int* slots, int n, int max_streams, int max_frames, int beam,
                                  float ins_bonus, int pad, int max_u, int* tokens, int* lengths, float* scores, int* stable_len,
                                  ea_stream_t stream);
/* Sub-word n-gram LM rows for the token-level beam searches (csrc/ngram_rows.hip) — the ARPA model the reference hands to
 * Flashlight's KenLM lexicon decoder (espresso/tools/ctc_decoder.py:24-71), queried here over the model's own dictionary
 * and fused as `lm_rows` by ea_ctc_prefix_beam_* and ea_rnnt_frame_beam_* (offline and streamed), as the LSTM LM's rows are.
 * `handle` is an uploaded ea_ngram_create handle of order n; W = n - 1; a context is int32 [W], oldest first, front-padded
 * with -1 (the convention of ea_ngram_score).  tok2word int32 [V] maps a dictionary id to an ARPA word id (>= 0), to -1 (no
 * ARPA entry: scores as <unk>, -inf without one) or to -2 (a column that is always -inf: pad, blank); no two ids share a word.
 * ea_ngram_token_map_create: checks such a host array, uploads it with its inverse (word2tok) to the current device and
 *   writes an opaque handle to *(void**)map_host (-2: bad map); the `tok2word` argument of the two device calls below is such
 *   a handle.  ea_ngram_token_map_destroy frees it.
 * ea_ngram_token_rows_step: one launch for N rows (one workgroup each).  Row i continues row parent[i] of ctx_in: with
 *   keep[i] (uint8) its context c is ctx_in[parent[i]], otherwise that context shifted left by one with word(token[i])
 *   appended; word(t) = tok2word[t] if >= 0, else the file's <unk>, else the id n1 that matches no n-gram.  ctx_out[i] = c
 *   (ctx_in != ctx_out: rows are gathered by parent), and rows[i * ld + v], fp32, ld >= V, is bit for bit what
 *   ea_ngram_score returns for (c, tok2word[v]), v < V; -2 columns are -inf.  Every row is recomputed, kept ones included.
 *   n == 1 (W == 0): the context pointers are not read.  A parent outside [0, N) is not reported (nothing is read back): the
 *   row then continues its own index, so that no launch reads outside ctx_in; a token outside [0, V) counts as one without
 *   an ARPA entry.
 * ea_ngram_token_rows_start: the context [-1, ..., -1, <s>] and its row, written to all N rows of ctx and rows.
 * ea_ngram_token_rows_host: the same contract on the host tables and host arrays (tok2word_host the int32 [V] array itself;
 *   parent_host == NULL: the start rows); a loop of single queries, for tests and as the kernel's yardstick. */
int ea_ngram_token_map_create(const void* handle, const int* tok2word_host, int V, void* map_host);
int ea_ngram_token_map_destroy(void* map);
int ea_ngram_token_rows_step(const void* handle, const void* tok2word, int V, const int* ctx_in, const int* parent,
                             const int* token, const void* keep, int N, int* ctx_out, float* rows, long ld, ea_stream_t stream);
int ea_ngram_token_rows_start(const void* handle, const void* tok2word, int V, int N, int* ctx, float* rows, long ld,
                              ea_stream_t stream);
int ea_ngram_token_rows_host(const void* handle, const int* tok2word_host, int V, const int* ctx_in_host, const int* parent_host,
                             const int* token_host, const void* keep_host, int N, int* ctx_out_host, float* rows_host, long ld);
/* Label-smoothed CE — espresso/criterions/label_smoothed_cross_entropy_v2.py:49-119.  smoothing 0 = uniform, 1 = unigram
 * (prior fp32 [V], sums to one), 2 = temporal (neighbouring targets of the same sentence, weights 2:5:5:2; rows are
 * b*tgt_len + u).  out_loss[0] += sum loss, out_loss[1] += sum nll (pad rows skipped). */
int ea_label_smoothed_ce(const void* logits, long ld, int logits_bf16, const int* target, float* out_loss,
                         void* dlogits, long ld_out, int dlogits_bf16, long M, int V, int pad_idx, float eps,
                         float grad_scale, int smoothing, const float* prior, int tgt_len, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Front-end: Kaldi fbank + global CMVN + SpecAugment + padding — espresso/tools/utils.py:426-454
 * (torchaudio.compliance.kaldi.fbank defaults), fairseq/data/audio/feature_transforms/global_cmvn.py:26-29,
 * espresso/data/feature_transforms/adaptive_specaugment.py:77-136, espresso/tools/utils.py:97-113.
 * wav: concatenated fp32 samples (int16 scale), offsets int64 [B+1]; feat fp32 [B][Tmax][nmel]
 * (rows >= n_frames(b) are written as 0); utt_sum fp32 [B] zeroed by caller (sum of features, for
 * the mean mask value); out_len int32 [B] = 1+(N-frame_len)/frame_shift.  window/twiddle/mel_* are
 * host-built tables (espresso_amd/data/fbank_tables.py).  Mask lists: int32 [B][n][2] = (start,width).
 * Tmax below an utterance's frame count: rows >= Tmax are neither stored nor summed into utt_sum, out_len still holds
 * the utterance's full count (not clamped: clamp it before it is used as a row bound).  Tmax <= 0: feat and utt_sum are
 * untouched and out_len is set to 0.  B <= 0 returns 0, frame_len > 512 or nmel > 128 returns -2; no output is written.
 * ea_specaugment clips nothing: lengths[b] <= Tmax and every mask inside [0, lengths[b]) x [0, nmel) are the caller's. */
int ea_fbank_batch(const float* wav, const long* offsets, int B, const float* window, const float* twiddle,
                   const int* mel_start, const int* mel_len, const int* mel_woff, const float* mel_w,
                   const float* cmvn_mean, const float* cmvn_std, float* feat, float* utt_sum, int* out_len,
                   int Tmax, int nmel, int frame_len, int frame_shift, float preemph, float log_floor,
                   ea_stream_t stream);
/* the same on int16 samples (what ea_audio_read_batch_i16 delivers): the conversion to fp32 is exact, half the bytes move */
int ea_fbank_batch_i16(const int16_t* wav, const long* offsets, int B, const float* window, const float* twiddle,
                   const int* mel_start, const int* mel_len, const int* mel_woff, const float* mel_w,
                   const float* cmvn_mean, const float* cmvn_std, float* feat, float* utt_sum, int* out_len,
                   int Tmax, int nmel, int frame_len, int frame_shift, float preemph, float log_floor,
                   ea_stream_t stream);
int ea_specaugment(float* feat, const int* lengths, const float* utt_sum, const int* fmask, const int* tmask,
                   int nf, int nt, int B, int Tmax, int nmel, int use_mean, float mask_value, ea_stream_t stream);

/* Polyphase resampler in front of the fbank (csrc/resample.hip; the Hann-windowed sinc of Kaldi's LinearResample, built on the
 * host by espresso_amd/data/resample.py): taps fp32 [phases][K], first int32 [phases].  Output j (ABSOLUTE index) has phase
 * p = j % phases and unit u = j / phases, and is  y[j] = sum_k taps[p][k] * x[first[p] + u * in_unit + k]  with
 * acc = +0; for k ascending: acc = fmaf(taps[p][k], x_k, acc)  in fp32 — the same bits for an utterance resampled at once and
 * in pieces.  in: concatenated samples, in_offsets int64 [B+1]; in_base int64 [B] = absolute index of the first sample held
 * for utterance b (samples outside [in_base[b], in_base[b] + len_b) read as 0); out fp32, out_offsets int64 [B+1] = where and
 * how many, out_base int64 [B] = absolute index of the first output to produce.  NULL bases mean 0 (offline).  max_out >= the
 * largest output count.  One launch, no host synchronisation, no atomics.  B <= 0 or max_out <= 0 returns 0; K outside
 * [1, 4096], phases <= 0, in_unit <= 0 or B > 65535 returns -2; no output is written in either case. */
int ea_resample_batch(const float* in, const long* in_offsets, const long* in_base, float* out, const long* out_offsets,
                      const long* out_base, int B, const float* taps, const int* first, int phases, int K, int in_unit,
                      long max_out, ea_stream_t stream);
/* the same on int16 samples: the conversion to fp32 is exact, the outputs are bit-identical */
int ea_resample_batch_i16(const int16_t* in, const long* in_offsets, const long* in_base, float* out, const long* out_offsets,
                      const long* out_base, int B, const float* taps, const int* first, int phases, int K, int in_unit,
                      long max_out, ea_stream_t stream);

/* Global CMVN statistics on the device — espresso/tools/compute_global_cmvn_stats.py:55-120 (per-utterance numpy
 * sum / variance merged on the host).  acc fp64 [2*nmel+1] = (sum[f], sum of squares[f], frame count), accumulated
 * across calls over the valid frames (t < lengths[b]) of feat fp32 [B][Tmax][nmel]; zeroed by the caller once. */
int ea_feature_stats(const float* feat, const int* lengths, double* acc, int B, int Tmax, int nmel, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer on flat fp32 buffers — fairseq/utils.py:347-397 (clip_grad_norm_),
 * fairseq/optim/adam.py:215-240.  coef[0] multiplies every gradient (pre_scale * clip), coef[1]
 * receives the (pre-scaled) gradient norm; both stay on the device.  ea_grad_sumsq ADDS to out.
 * A non-finite norm (sumsq inf or NaN, or a non-finite scale) gives a non-finite coef[0] as well.  ea_adam_step with a
 * non-finite coef[0] skips the update: p, m, v keep their bits, p_bf16 (if given) is still written as bf16(p), and g is
 * still zeroed when zero_grad is set (the overflowed gradient is discarded).  coef == NULL: the gradient is taken as is;
 * max_norm <= 0: no clipping.  Weight decay is decoupled: p += p * (-weight_decay * lr) before the Adam update. */
int ea_grad_sumsq(const float* g, long n, float* out, ea_stream_t stream);
/* scale = pre_scale / denom_dev[0] (denom_dev: device fp32 scalar such as the all-reduced sample_size; may be NULL) */
int ea_clip_coef(const float* sumsq, float pre_scale, const float* denom_dev, float max_norm, float* coef,
                 ea_stream_t stream);
/* ea_clip_coef, and sumsq[0] = 0 afterwards: the accumulator is ready for the next ea_grad_sumsq without a fill launch */
int ea_clip_coef_clear(float* sumsq, float pre_scale, const float* denom_dev, float max_norm, float* coef,
                       ea_stream_t stream);
int ea_adam_step(float* p, float* g, float* m, float* v, void* p_bf16, long n, const float* coef, float lr,
                 float beta1, float beta2, float eps, float weight_decay, int step, int zero_grad,
                 ea_stream_t stream);
/* ea_adam_step from a persistent grid of at most max_blocks (>= 1) workgroups, for a launch that shares the device with
 * another queue's kernels: same arguments, same kernel, bit-identical p, g, m, v and p_bf16.  A sub-range of the flat
 * buffers is addressed by offsetting the five pointers alike (by a multiple of 4 elements: 16-byte loads, and the bits
 * of an element depend on its lane of the float4). */
int ea_adam_step_capped(float* p, float* g, float* m, float* v, void* p_bf16, long n, const float* coef, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int step, int zero_grad,
                        int max_blocks, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Native layer runtime (csrc/engine.hip): a whole Conformer encoder layer per call —
 * espresso/modules/conformer_with_relative_positional_embedding_encoder_layer.py:81-145 forward and its
 * backward — as one back-to-back launch sequence on `stream`.  Weights: bf16 matrices (w1, w2, wqkv =
 * [q;k;v] rows, wo, wpos, pw1, pw2) + fp32 vectors; gradients are ACCUMULATED (+=) into the fp32
 * buffers in `grads` (the flat gradient buffer).  x: bf16 [B*T][C] batch-major rows.  `pe`: bf16
 * [2T-1][C] sinusoidal table.  `saved` carries activations from fwd to bwd, `scratch` is reusable;
 * sizes from ea_conformer_layer_workspace; fwd / bwd get the capacities of the two arenas and return -5 before
 * launching anything when an arena is too small.  Dropout masks are re-derived from `seed`. */
typedef struct EaFfnParams { const float *ln_g, *ln_b; const void* w1; const float* b1; const void* w2; const float* b2; } EaFfnParams;
typedef struct EaFfnGrads { float *ln_g, *ln_b, *w1, *b1, *w2, *b2; } EaFfnGrads;
typedef struct EaAttnParams {
  const float *ln_g, *ln_b; const void* wqkv; const float* bqkv; const void* wo; const float* bo;
  const float *pos_u, *pos_v; const void* wpos;
} EaAttnParams;
typedef struct EaAttnGrads { float *ln_g, *ln_b, *wqkv, *bqkv, *wo, *bo, *pos_u, *pos_v, *wpos; } EaAttnGrads;
typedef struct EaConvParams {
  const float *ln_g, *ln_b; const void* pw1; const float* dw; const float *bn_g, *bn_b; float *bn_rm, *bn_rv; const void* pw2;
} EaConvParams;
typedef struct EaConvGrads { float *ln_g, *ln_b, *pw1, *dw, *bn_g, *bn_b, *pw2; } EaConvGrads;
typedef struct EaLayerGrads { EaFfnGrads ffn1; EaAttnGrads attn; EaConvGrads conv; EaFfnGrads ffn2; float *final_ln_g, *final_ln_b; } EaLayerGrads;
typedef struct EaConformerLayer {
  EaFfnParams ffn1; EaAttnParams attn; EaConvParams conv; EaFfnParams ffn2; const float *final_ln_g, *final_ln_b;
  EaLayerGrads grads;
  /* optional (may be NULL): bf16 scratch of 4*C*F + 7*C*C elements owned by the caller.  A training forward refreshes it with
   * the transposes of ffn1.w1, ffn2.w1, wqkv, wo, pw1, pw2, ffn1.w2, ffn2.w2 (in this order); the backward's data-gradient
   * GEMMs then read k-contiguous weights (direct-to-LDS kernel where it pays) instead of transposing them in registers. */
  void* wt;
} EaConformerLayer;
typedef struct EaLayerShape {
  int B, T, C, H, F, KW, training; float p_drop, p_act, p_attn; uint64_t seed; int has_attn_mask;
  /* backward only: the scratch arena is untouched since the previous ea_conformer_layer_bwd call with the same shape and
   * settings (consecutive layers of one backward pass) - lets the attention backward skip re-zeroing its band buffer */
  int scratch_clean;
  /* relative-position mode of the attention block: 0 = sinusoidal table projected by pos_proj with pos_bias_u / pos_bias_v (the
   * Conformer recipes), 1 = learned table (`pe` is the bf16 [2T-1][C] slice of the table, used as is; its fp32 gradient is
   * returned through `dpe`).  `act`: FFN activation of the Transformer layer (EA_ACT_RELU / EA_ACT_SILU); the Conformer
   * layer always uses SiLU. */
  int pos_mode, act;
  int S; /* decoder layer only: padded encoder length (keys of the encoder-decoder attention); T is then the target length */
  /* backward only (conformer / transformer encoder layers): 0 = the call returns with every gradient ordered on `stream`
   * (side work forked and joined inside the call); 1 or 2 = DEFERRED mode using scratch half (defer - 1): the optimizer-only
   * work (all weight / bias / LayerNorm / BatchNorm parameter gradients) is launched on the side stream at the end of the call
   * and joined by the next backward call, which must use the other half — so it overlaps that call's data-gradient chain.
   * The gradients of a deferred call are ordered on `stream` once the NEXT backward call, ea_backward_flush or any layer
   * forward call has been issued; `saved` must stay alive until then. */
  int defer;
  /* forward only (Conformer layer, training): 1 = the k-contiguous weight copies in EaConformerLayer.wt are already fresh for this
   * update (the caller ran ea_conformer_layer_refresh_wt after the optimizer step, typically on another stream under the
   * sub-sampler's forward pass) - the forward call then skips its own transposes.  0 = the call refreshes them itself. */
  int wt_fresh;
  /* Conformer layer: 1 = the convolution module's depthwise convolution is causal (ea_glu_dwconv_causal_*: left pad KW-1, no
   * look-ahead; encoder.depthwise_conv_causal), 0 = the reference's symmetric one. */
  int conv_causal;
} EaLayerShape;

/* Dropout sites of a layer call (FairseqDropout calls of the reference, cited per site) and the mask stream each one uses.
 * Every site keeps element `idx` iff ea_dropout_hash(site seed, idx) >= thr, thr = min(floor(p * 2^32), 2^32 - 1), and scales
 * kept elements by 1 / (1 - p); site seed = ea_layer_dropout_seed(EaLayerShape.seed, site).  Element index per site, with
 * activation rows m = b*T + t (batch-major):
 *   *_ACT    m*F + f        fairseq/modules/conformer_layer.py:144 / transformer_layer.py:212 (activation_dropout, after the activation)
 *   *_OUT    m*C + c        conformer_layer.py:146 / transformer_layer.py:216 (dropout on the FFN output, before 0.5*y + x)
 *   *_PROBS  ((h*B + b)*T + i)*S + j   fairseq/modules/multihead_attention.py:874 (attention_dropout on the softmax output)
 *   ATTN_OUT / CROSS_OUT  m*C + c      espresso/modules/conformer_with_relative_positional_embedding_encoder_layer.py:125,
 *                                      transformer_layer.py:196, 456, 481 (dropout on out_proj's output, before the residual)
 *   CONV_OUT m*C + c        conformer_layer.py:100 (dropout at the end of the convolution module)
 * The Transformer encoder / decoder layers use FFN1_* for their one FFN; CROSS_* exist in the decoder layer only. */
enum {
  EA_SITE_FFN1_ACT = 0, EA_SITE_FFN1_OUT = 1, EA_SITE_ATTN_PROBS = 2, EA_SITE_ATTN_OUT = 3, EA_SITE_CONV_OUT = 4,
  EA_SITE_FFN2_ACT = 5, EA_SITE_FFN2_OUT = 6, EA_SITE_CROSS_PROBS = 7, EA_SITE_CROSS_OUT = 8
};
uint64_t ea_layer_dropout_seed(uint64_t layer_seed, int site);
/* Host evaluation of the device's counter-based dropout hash (csrc/common.h ea_hash) for idx0 .. idx0 + n - 1: the pin for
 * the tests' numpy restatement (oracle/dropout_ref.py); no GPU needed. */
int ea_dropout_hash_host(uint64_t seed, uint64_t idx0, long n, uint32_t* out);

/* tuning hook: run weight-gradient GEMMs / bias sums of the layer backward on a side stream (default on); returns the
 * previous value.  Sizes from ea_conformer_layer_workspace depend on this setting: query them after changing it. */
int ea_set_backward_overlap(int on);
/* tuning hook: honour EaLayerShape.defer (default on); returns the previous value.  Workspace sizes depend on it. */
int ea_set_backward_deferred(int on);
/* tuning hook (A/B): run the deferred work on the caller's stream at the end of each layer backward instead of the side stream */
int ea_set_backward_deferred_inline(int on);
/* make `stream` wait for all deferred side work issued so far (call after the last layer backward of a pass) */
int ea_backward_flush(ea_stream_t stream);
/* Do two streams share a HARDWARE queue?  1 = work on `b` waits for work on `a`, 0 = they run side by side, < 0 = error.
 * HIP deals a process's streams onto 4 hardware queues by load; two streams on one queue serialise silently.  The layer
 * runtime picks its side stream with this probe (a tiny kernel on `b` must finish while a 200 us spin kernel runs on `a`); callers
 * that create their own side streams can do the same.  Blocks the host until `a` reaches the probe; EA_SIDE_STREAM_PROBE=0
 * disables the runtime's own use of it. */
int ea_streams_share_queue(ea_stream_t a, ea_stream_t b);
/* What the probe decided for the layer runtime's own side stream (created by the first backward call): returns 1 when the stream
 * exists; *rejected = candidate streams that shared the caller's hardware queue and were turned down (-1: none created yet),
 * *unprobed = 1 when the accepted stream was not measured (EA_SIDE_STREAM_PROBE=0, or the eighth candidate).  Reported per rank in
 * the bench line: on a multi-rank job RCCL's streams change how HIP deals queues, so every rank's verdict should be visible. */
int ea_side_stream_report(int* rejected, int* unprobed);
int ea_conformer_layer_workspace(const EaLayerShape* shape, long* saved_bytes, long* scratch_bytes);
/* The k-contiguous (transposed) bf16 copies of a Conformer layer's eight weight matrices, which its BACKWARD data-gradient GEMMs
 * read (EaConformerLayer.wt): one batched transpose on `stream`.  The weights only change in the optimizer step, and nothing in the
 * forward pass reads the copies: a caller can refresh all layers on a side stream right after the optimizer step and pass
 * EaLayerShape.wt_fresh = 1 to the forward calls (12 launches off the compute stream per update step). */
int ea_conformer_layer_refresh_wt(const EaConformerLayer* layer, const EaLayerShape* shape, ea_stream_t stream);
int ea_conformer_layer_fwd(const EaConformerLayer* layer, const EaLayerShape* shape, const void* x_in, void* x_out,
                           const int* key_len, const float* attn_mask, const void* pe, void* saved, long saved_bytes,
                           void* scratch, long scratch_bytes, ea_stream_t stream);
int ea_conformer_layer_bwd(const EaConformerLayer* layer, const EaLayerShape* shape, const void* x_in, const void* dy,
                           void* dx, const int* key_len, const void* pe, void* saved, long saved_bytes, void* scratch,
                           long scratch_bytes, ea_stream_t stream);
/* CHAINED calls over a stack of Conformer layers of one shape (C <= 512): layer k's closing LayerNorm and layer k+1's opening
 * LayerNorm (of ffn1) touch the same rows back to back, in the forward and — mirrored — in the backward pass.  A chained call does
 * both with one kernel (ea_layernorm_fwd2 / ea_layernorm_bwd2_dx): 2 launches and two passes over the activations fewer per layer
 * boundary and update, results bit-identical to the plain calls.  All members may be NULL / 0 (= the plain call).
 *   forward of layer k:    `next` / `next_saved`: the following layer and ITS saved arena; this call also writes that layer's ffn1
 *                          LayerNorm output and statistics there.
 *   forward of layer k+1:  `ln1_done` = 1: `saved` already holds them (the previous call was chained to this layer).
 *   backward of layer k+1: `prev` / `prev_saved` / `prev_seed` (EaLayerShape.seed of layer k's forward) / `prev_pre` (bf16 [B*T][C]
 *                          buffer): the call ends with layer k's final-LayerNorm backward; `dx` receives the gradient w.r.t. layer
 *                          k's PRE-final-norm activations, `prev_pre` the 0.5 * dropout(.) copy layer k's ffn2 block starts from, and
 *                          layer k's final_ln gradients are accumulated with this call's side work.
 *   backward of layer k:   `final_ln_done` = 1: `dy` is that gradient and `pre_in` that copy; the call skips its final-norm backward.
 * The caller must hand layer k+1's `dx` to layer k unchanged (layer k's output has no other consumer), and `prev_pre` must stay
 * untouched until layer k's own side work has been joined (deferred mode: by the backward call AFTER layer k's, or by
 * ea_backward_flush) — its weight-gradient launch reads the buffer. */
typedef struct EaLayerChain {
  const EaConformerLayer* next; void* next_saved; long next_saved_bytes; int ln1_done;
  const EaConformerLayer* prev; void* prev_saved; long prev_saved_bytes; uint64_t prev_seed; void* prev_pre;
  int final_ln_done; const void* pre_in;
} EaLayerChain;
int ea_conformer_layer_fwd_chained(const EaConformerLayer* layer, const EaLayerShape* shape, const EaLayerChain* chain, const void* x_in,
                                   void* x_out, const int* key_len, const float* attn_mask, const void* pe, void* saved,
                                   long saved_bytes, void* scratch, long scratch_bytes, ea_stream_t stream);
int ea_conformer_layer_bwd_chained(const EaConformerLayer* layer, const EaLayerShape* shape, const EaLayerChain* chain, const void* x_in,
                                   const void* dy, void* dx, const int* key_len, const void* pe, void* saved, long saved_bytes,
                                   void* scratch, long scratch_bytes, ea_stream_t stream);
/* A STACK of n Conformer layers of one shape in one call per direction — the layer loop of
 * espresso/models/transformer/speech_transformer_encoder.py:374-390 and its backward.  Same launches as n chained layer calls
 * (`chain` != 0: EaLayerChain between consecutive members; 0: plain calls); what it saves is host time: at small batches (the
 * transducer recipe: ~1 500 rows per micro-batch) a layer call issued from the Python loop costs 142 us (forward) / 181 us (backward)
 * of host time against 64 us for the same call issued back to back from C (cold caches after the interpreter ran;
 * profiles/r06_transducer_host_split.txt).
 * L[k].x_in: bf16 [B*T][C] input of layer k — for k > 0 ALSO the output buffer of layer k-1; x_out: output of the last layer.
 * L[k].shape: the layer's own seed / wt_fresh; backward: its own `defer` (alternating halves as for consecutive plain calls) and
 * `scratch_clean`.  Backward: dy / dx of the stack; dbuf: two bf16 [B*T][C] buffers for the gradients between layers; pre: three
 * bf16 [B*T][C] buffers used in rotation for EaLayerChain.prev_pre (must stay untouched until ea_backward_flush / the next
 * backward call; ignored when chain == 0).  Gradient ordering on `stream`: as after the same sequence of layer calls (the last
 * member's deferred side work is joined by the next backward call or ea_backward_flush). */
typedef struct EaStackLayer { const EaConformerLayer* layer; EaLayerShape shape; void* saved; long saved_bytes; void* x_in; } EaStackLayer;
int ea_conformer_stack_fwd(const EaStackLayer* L, int n, void* x_out, const int* key_len, const float* attn_mask, const void* pe,
                           void* scratch, long scratch_bytes, int chain, ea_stream_t stream);
int ea_conformer_stack_bwd(const EaStackLayer* L, int n, const void* dy, void* dx, void* const* dbuf, void* const* pre,
                           const int* key_len, const void* pe, void* scratch, long scratch_bytes, int chain, ea_stream_t stream);
/* Transformer encoder layer (pre-LN; fairseq/modules/transformer_layer.py:135-214 with the rel-pos MHA of
 * multihead_attention.py:650-907) in the same runtime: uses the `attn` and `ffn1` members (+ their grads) of EaConformerLayer;
 * `wt` (optional) holds 2*C*F + 4*C*C bf16 elements.  dpe: fp32 [2T-1][C], required iff shape->pos_mode == 1. */
int ea_transformer_layer_workspace(const EaLayerShape* shape, long* saved_bytes, long* scratch_bytes);
int ea_transformer_layer_fwd(const EaConformerLayer* layer, const EaLayerShape* shape, const void* x_in, void* x_out,
                             const int* key_len, const float* attn_mask, const void* pe, void* saved, long saved_bytes,
                             void* scratch, long scratch_bytes, ea_stream_t stream);
int ea_transformer_layer_bwd(const EaConformerLayer* layer, const EaLayerShape* shape, const void* x_in, const void* dy,
                             void* dx, const int* key_len, const void* pe, float* dpe, void* saved, long saved_bytes,
                             void* scratch, long scratch_bytes, ea_stream_t stream);
/* Transformer DECODER layer (pre-LN; fairseq/modules/transformer_layer.py:241-529 as built by
 * espresso/modules/transformer_with_relative_positional_embedding_layer.py:66-116) for teacher-forced training: causal
 * self-attention, encoder-decoder attention over `enc` (bf16 [B*S][C], valid lengths enc_len), FFN.  Head dim 64 (fused
 * attention kernels).  x: bf16 [B*T][C].  denc: bf16 [B*S][C], this layer's gradient w.r.t. `enc` (written, not accumulated).
 * `wt` (optional): 2*C*F + 8*C*C bf16 elements for the k-contiguous weight copies. */
typedef struct EaXAttnParams { const float *ln_g, *ln_b; const void* wq; const float* bq; const void* wkv; const float* bkv; const void* wo; const float* bo; } EaXAttnParams;
typedef struct EaXAttnGrads { float *ln_g, *ln_b, *wq, *bq, *wkv, *bkv, *wo, *bo; } EaXAttnGrads;
typedef struct EaDecoderLayer {
  EaAttnParams self_attn; EaXAttnParams cross; EaFfnParams ffn;
  EaAttnGrads g_self; EaXAttnGrads g_cross; EaFfnGrads g_ffn;
  void* wt;
} EaDecoderLayer;
int ea_decoder_layer_workspace(const EaLayerShape* shape, long* saved_bytes, long* scratch_bytes);
int ea_decoder_layer_fwd(const EaDecoderLayer* layer, const EaLayerShape* shape, const void* x_in, const void* enc, void* x_out,
                         const int* enc_len, void* saved, long saved_bytes, void* scratch, long scratch_bytes, ea_stream_t stream);
int ea_decoder_layer_bwd(const EaDecoderLayer* layer, const EaLayerShape* shape, const void* x_in, const void* enc, const void* dy,
                         void* dx, void* denc, const int* enc_len, void* saved, long saved_bytes, void* scratch, long scratch_bytes,
                         ea_stream_t stream);
/* tuning / test hook: use the fused attention kernels inside the layer runtime when the shape allows (default on);
 * returns the previous value.  Workspace sizes depend on it. */
int ea_set_flash_attention(int on);
/* tuning / test hook: LayerNorm backward writes the next block's dropout-scaled gradient as a second output (default on) */
int ea_set_fused_predrop(int on);

/* ------------------------------------------------------------------------------------------
 * Look-ahead word LM fusion (csrc/lookahead.hip) — espresso/models/tensorized_lookahead_language_model.py:83-269 over the
 * tensorized prefix tree of espresso/tools/tensorized_prefix_tree.py:14-108 (int32 device copies: children [NN][D],
 * prev_subword [NN], word_idx [NN], word_set [NN][2]; node 0 = none, node 1 = root).
 * ea_softmax_cumsum: cumsum[n][v] = sum_{w<=v} softmax(logits[n])[w] (fp32, rows ld apart), lp_tok[n] = log softmax[n][tok];
 *   rows with row_mask[n] == 0 keep their previous values (row_mask NULL = all rows).
 * ea_lookahead_advance: nodes[n] <- root if prev_tok[n] == space else the child reached by prev_tok[n] (none if absent).
 * ea_lookahead_logprobs: out fp32 [N][Vs] = sub-word log-probabilities of Eqn. 15 (floor log(1e-10)); lp_word_eos[n] is used
 *   as the <eos> score of hypotheses whose last sub-word is <space>. */
int ea_softmax_cumsum(const float* logits, long ld, const uint8_t* row_mask, float* cumsum, float* lp_tok, int N, int V, int tok,
                      ea_stream_t stream);
int ea_lookahead_advance(int* nodes, const int* prev_tok, const int* children, const int* prev_subword, int N, int D,
                         int space_idx, int root_id, ea_stream_t stream);
int ea_lookahead_logprobs(const int* nodes, const int* prev_tok, const float* cumsum, const float* lp_word_eos, const int* children,
                          const int* prev_subword, const int* word_idx, const int* word_set, float* out, int N, int Vw, int Vs,
                          int D, float oov_penalty, int open_vocab, int word_unk, int sub_space, int sub_eos, int sub_pad,
                          ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Multi-level (sub-word + word) LM fusion (csrc/multilevel.hip) — espresso/models/external_language_model.py:376-552 over the
 * same int32 tree tensors as the look-ahead kernels (children [NN][D], prev_subword [NN], word_idx [NN]; node 0 = none).
 * ea_multilevel_lm_step: one beam step after both LMs' output GEMMs (fp32 logits, rows ldw / lds apart).
 *   word_lp fp32 [N][Vw] <- log_softmax(word_logits) on the first call and where prev_tok == sub_space, else kept;
 *   nodes int32 [N] <- tree transition on prev_tok (root on the first call); cum fp32 [N] <- running sub-word score of the
 *   current word, accumulated from prev_out fp32 [N][Vs] (the previous call's out; NULL on the first call);
 *   out fp32 [N][Vs] = subword_weight * log_softmax(sub_logits) with the <space> column replaced by the word score and the
 *   closed-vocabulary / <space> / <eos> masks (logzero = -10). */
int ea_multilevel_lm_step(const float* word_logits, long ldw, const float* sub_logits, long lds, const int* prev_tok,
                          const float* prev_out, float* word_lp, float* cum, int* nodes, float* out, const int* children,
                          const int* prev_subword, const int* word_idx, int N, int Vw, int Vs, int D, float subword_weight,
                          float log_oov_penalty, int first, int open_vocab, int word_eos, int word_unk, int sub_space, int sub_eos,
                          int root_id, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * LSTM cell element-wise stages (csrc/lstm.hip) — torch.nn.LSTMCell as driven by espresso/models/speech_lstm.py:846-893
 * (transducer predictor, LSTM LM, attention decoder).  The packed pre-activations gates_pre = x W_ih^T + b_ih + h W_hh^T
 * + b_hh ([B][ldg] fp32, gate order i,f,g,o) come from ea_gemm_bf16 (fp32 output, fp32 residual).
 *   fwd: c_out/h fp32 [B][H]; h_out_bf16 [B][ldh] (GEMM operand of the next step / layer); gates_act fp32 [B][4H] saved for
 *        bwd (NULL at inference); keep_row uint8 [B] (NULL = none): rows whose state is frozen (h_prev_f32 required).
 *   bwd: dh = dh_bf16 (from the layer above, [B][ld_dh], may be NULL) + dh_f32 (recurrent, may be NULL); dc_in may be NULL;
 *        dgates bf16 [B][lddg]; dc_prev fp32 [B][H].
 * ea_gather_rows: out[n] = in[parent[n]] over rows of W elements of 2 or 4 bytes (beam reorder of cached LSTM states,
 * speech_lstm.py:981-999). */
int ea_lstm_cell_fwd(const float* gates_pre, long ldg, const float* c_prev, float* c_out, float* h_out_f32, void* h_out_bf16,
                     long ldh, float* gates_act, const uint8_t* keep_row, const float* h_prev_f32, int frozen_out_zero, int B,
                     int H, ea_stream_t stream);
int ea_lstm_cell_bwd(const void* dh_bf16, long ld_dh, const float* dh_f32, const float* dc_in, const float* gates_act,
                     const float* c_prev, const float* c, void* dgates, long lddg, float* dc_prev, const uint8_t* frozen, int B,
                     int H, ea_stream_t stream);
/* Whole time loop of one LSTM layer in one persistent launch (csrc/lstm_seq.hip) — the LSTMCell loop of
 * espresso/models/speech_lstm.py:846-893 and one direction of the packed nn.LSTM of :470-520.  Recurrent weights stay in
 * registers, workgroups exchange h_t (fwd) / dgates_t (bwd) through global memory behind a grid barrier per step.
 *   gx fp32 [U*B][4H] = x W_ih^T + b_ih + b_hh (rows t*B + b); w_hh bf16 [4H][H]; w_hhT bf16 [H][4H]; h0 bf16 [B][H] / c0 fp32
 *   [B][H] (NULL = zero state); frozen uint8 [U][B] (NULL = none); reverse: walk t = U-1 .. 0.
 *   fwd out: hs bf16 [U*B][H], cs fp32 [U][B][H], act fp32 [U][B][4H] (activated gates i,f,g,o), h_last fp32 [B][H] (may be NULL).
 *   bwd in : dhs bf16 [U*B][H] (may be NULL), dh_last / dc_last fp32 [B][H] (may be NULL);
 *   bwd out: dG bf16 [U*B][4H] (gradient of the gate pre-activations), dh0 / dc0 fp32 [B][H] (may be NULL).
 *   counter: 2 x uint32 of device scratch (zeroed by the call); counter[1] != 0 afterwards = a barrier wait timed out.
 * ea_lstm_seq_supported: 1 <= B <= 64 and H in {256, 320, 512, 640, 768, 800, 1024}; other shapes return -2 (callers use
 * the per-step ea_gemm_bf16 + ea_lstm_cell_* path). */
int ea_lstm_seq_supported(int B, int H);
int ea_lstm_seq_fwd(const float* gx, const void* w_hh, const void* h0, const float* c0, const uint8_t* frozen, void* hs, float* cs,
                    float* act, float* h_last, unsigned* counter, int B, int U, int H, int reverse, int frozen_out_zero,
                    ea_stream_t stream);
int ea_lstm_seq_bwd(const void* dhs, const float* dh_last, const float* dc_last, const float* act, const float* cs, const float* c0,
                    const uint8_t* frozen, const void* w_hhT, void* dG, float* dh0, float* dc0, unsigned* counter, int B, int U,
                    int H, int reverse, ea_stream_t stream);
/* frozen_out_zero / frozen: packed-sequence semantics of the BiLSTM encoder (speech_lstm.py:470-520, pack_padded_sequence /
 * pad_packed_sequence with padding_value 0): rows past their length keep their state, emit zeros and get no gradient.
 *
 * Bahdanau attention of one decoder step — espresso/modules/speech_attention.py:38-87 (normalize=True):
 *   score[t][b] = sum_a nv[a] tanh(qp[b][a] + key[t][b][a] + bias[a]), nv = g v/||v|| (caller), softmax over t < len[b],
 *   ctx[b] = sum_t p[t][b] value[t][b] (len[b] == 0: p = 0, ctx = 0).  qp bf16 [B][A]; key bf16 [T][B][A]; value bf16 [T][B][Cv]; p fp32 [T][B]; ctx bf16 [B][ldc].
 * bwd (one step): dqp bf16 [B][A]; dkey_acc fp32 [T][B][A] and dvalue_acc fp32 [T][B][Cv] are accumulated in place over the
 * decoder steps; dnv_acc / dbias_acc fp32 [A] by atomics. */
int ea_bahdanau_fwd(const void* qp, const void* key, const void* value, const float* nv, const float* bias, const int* len,
                    float* p_out, void* ctx, long ldc, int T, int B, int A, int Cv, const int* kv_col, int Bkv,
                    ea_stream_t stream);
/* kv_col (int [B], or NULL): beam search — row b attends over column kv_col[b] of key / value / len, which then have Bkv
 * columns (one per sentence) instead of B. */
int ea_bahdanau_bwd(const void* dctx, long ldd, const void* qp, const void* key, const void* value, const float* nv,
                    const float* bias, const int* len, const float* p, void* dqp, float* dkey_acc, float* dvalue_acc,
                    float* dnv_acc, float* dbias_acc, int T, int B, int A, int Cv, ea_stream_t stream);
int ea_gather_rows(const void* in, void* out, const int* parent, int N, int W, int elem_bytes, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batched beam-search decoding (csrc/decode.hip) — fairseq/sequence_generator.py:355-609, fairseq/search.py:103-144,
 * fairseq/modules/multihead_attention.py:716-760,878-897,964-989.
 * ea_decode_attention: out[n] = softmax(q[n] . K[r]^T) V[r], r = kv_row ? kv_row[n] : n, over len ? len[r] : max_len keys;
 *   q/out bf16 [N][ldq] (q pre-scaled), K/V bf16 rows of `row_stride` elements, key j at j*ldkv + koff/voff + h*dh.
 *   len[r] <= max_len; a row with len[r] == 0 attends to nothing: out[n] = 0 (and probs = 0).
 * ea_kv_append_reorder: new[n][0:L] = old[parent[n]][0:L], new[n][L] = kv_new[n]  (rows of W bf16, capacity Lmax).
 * ea_beam_mask_rows: sequence_generator.py:395-424 on fp32 lprobs [N][V] in place.
 * ea_beam_topk: per sentence the k (<=128) best of lprobs[(s*beam+b)][v] + prev_scores[s*beam+b], b < nbeam_used. */
int ea_decode_attention(const void* q, const void* K, const void* V, const int* kv_row, const int* len, void* out, int N, int H,
                        int dh, long ldq, long row_stride, long ldkv, int koff, int voff, int max_len, ea_stream_t stream);
int ea_kv_append_reorder(const void* old_cache, void* new_cache, const void* kv_new, const int* parent, int N, int L, int Lmax,
                         int W, ea_stream_t stream);
/* ea_decode_attention_probs: ea_decode_attention (same `out`, bit for bit) that also writes fp32 probs[(n*H + h)*ldp + j]
 *   = softmax weight of key j for j < len, 0 for len <= j < max_len (ldp >= max_len).
 * ea_attn_history_put: dst[n*ldd + j] = ((accumulate ? dst : 0) + mean_h src[n*s_row + j*s_frame + h*s_head]) / div, n < N, j < S.
 * ea_attn_backtrace: for i < n: rows_step = bbsz[i], rows_{k-1} = P[k*ldp + rows_k];
 *   out[(i*S + s)*(step+1) + k] = A[k*slab + rows_k*lda + s]  (fp32 alignment [S][step+1] of every finalized hypothesis). */
int ea_decode_attention_probs(const void* q, const void* K, const void* V, const int* kv_row, const int* len, void* out, int N, int H,
                              int dh, long ldq, long row_stride, long ldkv, int koff, int voff, int max_len, float* probs, long ldp,
                              ea_stream_t stream);
int ea_attn_history_put(const float* src, long s_row, long s_frame, long s_head, int N, int H, int S, float* dst, long ldd,
                        int accumulate, float div, ea_stream_t stream);
int ea_attn_backtrace(const float* A, long slab, long lda, const int* P, long ldp, const long* bbsz, int n, int step, int S,
                      float* out, ea_stream_t stream);
int ea_beam_mask_rows(float* lprobs, int N, int V, int pad, int unk, int eos, float unk_penalty, int only_eos, int forbid_eos,
                      float eos_factor, int use_eos_factor, ea_stream_t stream);
int ea_beam_topk(const float* lprobs, const float* prev_scores, int bsz, int beam, int nbeam_used, int V, int k,
                 float* cand_score, int* cand_tok, int* cand_beam, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * RNN-T loss — torchaudio.functional.rnnt_loss as called at espresso/criterions/transducer_loss.py:130-140
 * (blank = "<s>", clamp = -1, fused log-softmax).  logits fp32 or bf16 (logits_bf16) [B][T][U1][V] (U1 = Umax + 1; bf16 is
 * what the reference's fc_out produces under bf16 autocast), targets int32 [B][Umax], loss fp32 [B] = -log p(y|x);
 * grad = grad_scale * d(sum loss)/d(logits), fp32 or bf16, same layout as logits.
 * ld: row pitch of logits AND grad in elements (>= V).  The joint of this library writes rows padded to a multiple of 64
 * (V = 5004 -> 5056): 16-byte accesses here, aligned fast paths / direct-to-LDS GEMMs for the three joint products; the grad
 * kernel writes the pad columns as zeros so that they can be part of a GEMM reduction.
 * workspace: ea_rnnt_workspace_bytes(B,T,U1) bytes, kept between the two calls. */
long ea_rnnt_workspace_bytes(int B, int T, int U1);
int ea_rnnt_loss(const void* logits, int logits_bf16, const int* targets, const int* logit_lengths, const int* target_lengths,
                 float* loss, void* workspace, int B, int T, int U1, int V, long ld, int Umax, int blank, ea_stream_t stream);
int ea_rnnt_grad(const void* logits, int logits_bf16, const int* targets, const int* logit_lengths, const int* target_lengths,
                 const float* loss, const void* workspace, void* grad, int grad_bf16, int B, int T, int U1, int V, long ld,
                 int Umax, int blank, float grad_scale, const float* grad_scale_dev, ea_stream_t stream);
/* The alpha / beta sweep of ea_rnnt_loss alone: lpb / lpy fp32 [B][T][U1] = log p(blank | t,u), log p(y_{u+1} | t,u). */
int ea_rnnt_scan(const float* lpb, const float* lpy, const int* logit_lengths, const int* target_lengths, float* alpha,
                 float* beta, float* loss, int B, int T, int U1, ea_stream_t stream);
/* Joint output layer FUSED with the RNN-T loss (csrc/joint_rnnt.hip, round 6): replaces fc_out of
 * espresso/models/transformer/speech_transformer_transducer_base.py:276-299 followed by torchaudio.functional.rnnt_loss
 * (espresso/criterions/transducer_loss.py:130-140) without ever writing the (B, T, U1, V) logits.
 *   Z bf16 [B*T*U1][J] = relu(E + D) (ea_joint_add_relu_f32), W bf16 [V][J], bias fp32 [V] or NULL; J % 64 == 0, 16-byte aligned.
 * ea_joint_rnnt_loss: loss[b] as ea_rnnt_loss, computed from the fp32 accumulators of the product (the unfused path rounds the
 *   logits to bf16 first); the workspace keeps lse / log-probs / alpha / beta for the gradient call.
 * ea_joint_rnnt_grad: dl bf16 [B*T*U1][ld] = d loss / d logits * grad_scale (* grad_scale_dev[0]); ld % 32 == 0, ld >= V, columns
 *   V .. ld - 1 are written as zeros (dl is the operand of the joint's data- and weight-gradient GEMMs, which reduce over ld).
 * Both return -2 for shapes they do not take (the caller then materialises the logits and uses ea_rnnt_loss / ea_rnnt_grad). */
long ea_joint_rnnt_workspace_bytes(int B, int T, int U1, int V);
int ea_joint_rnnt_loss(const void* Z, const void* W, const float* bias, const int* targets, const int* logit_lengths,
                       const int* target_lengths, float* loss, void* workspace, int B, int T, int U1, int V, int J, int Umax,
                       int blank, ea_stream_t stream);
int ea_joint_rnnt_grad(const void* Z, const void* W, const float* bias, const int* targets, const int* logit_lengths,
                       const int* target_lengths, const float* loss, void* workspace, void* dl, long ld, int B, int T, int U1,
                       int V, int J, int Umax, int blank, float grad_scale, const float* grad_scale_dev, ea_stream_t stream);
/* Where the transducer lattice sits after a loss call: byte offset of lpb (which = 0) or lpy (which = 1), fp32 [B][T][U1] with
 * the meaning of ea_rnnt_scan's, inside the workspace of ea_joint_rnnt_loss (..._joint_...) or of ea_rnnt_loss; -1 for another
 * `which`.  The forced aligner reads the lattice there (no change to what the loss calls compute). */
long ea_joint_rnnt_lattice_offset(int B, int T, int U1, int V, int which);
long ea_rnnt_lattice_offset(int B, int T, int U1, int which);

/* ------------------------------------------------------------------------------------------
 * Forced alignment (csrc/align.hip): the Viterbi (max-plus) twins of the CTC and RNN-T scans plus a backtrace, for a known
 * transcript.  The reference aligns only through Kaldi (estimate_initial_state_prior_from_alignments.py); the greedy CTC
 * timesteps of espresso/tools/ctc_decoder.py:171-186 belong to the hypothesis.  One workgroup per utterance; outputs stay on
 * the device (no host synchronisation).
 *
 * ea_ctc_viterbi_align: x fp32 or bf16 (x_bf16) [B][T][ld] log-probs (ld >= V), targets int32 [B][Lmax], in_len / tgt_len int32
 *   [B] (clamped to T / Lmax), workspace: ea_ctc_viterbi_workspace_bytes(B, T, Lmax) bytes, any contents.
 *   Lattice: blank y1 blank ... yU blank (S = 2U + 1 states); moves stay, +1, +2 (+2 only into a non-blank state whose label
 *   differs from the label two states earlier); a path starts in state 0 or 1 and ends in state S-1 or S-2.
 *   TIE RULE: stay over +1 over +2 (from the predecessor's side: the backtrace takes the first of s, s-1, s-2 with the maximum);
 *   at the end S-1 over S-2.
 *   Outputs: tok_start / tok_end int32 [B][Lmax] = first frame of token u's non-blank run and one past its last frame (trailing
 *   blanks are not part of a token; -1 for u >= U); frame_label int32 [B][T] = u on a frame of token u, -1 on blank frames, -2
 *   from in_len on; score fp32 [B] = sum of the chosen log-probs (U == 0: the all-blank path; in_len == U == 0: 0).
 *   Infeasible utterances (in_len < U + number of equal adjacent targets, or a lattice with no finite path): score = -inf,
 *   tok_start = tok_end = -1, frame_label = -2.  A target id outside [0, V) or equal to blank cannot be returned as an error
 *   without reading device memory on the host: that utterance gets score = NaN and the -1 / -2 fill, and is not aligned.
 *   Returns -2 for S > 2048 (Lmax > 1023), Lmax < 1, ld < V or blank outside [0, V).
 * ea_rnnt_viterbi_align: lpb / lpy fp32 [B][T][U1] as in ea_rnnt_scan (log p(blank | t,u), log p(y_{u+1} | t,u)),
 *   logit_lengths / target_lengths int32 [B], workspace: ea_rnnt_viterbi_workspace_bytes(B, T, U1) bytes, any contents.
 *   From node (t,u) the path takes blank to (t+1,u) or emits y_{u+1} to (t,u+1); it ends with the blank out of (T_b-1, U_b).
 *   TIE RULE: emit over blank at the node where the choice is made (the earlier emission).
 *   Outputs: emit_frame int32 [B][U1-1] = the frame at which token u is emitted (-1 for u >= U_b); score fp32 [B] = sum of
 *   the chosen log-probs (-inf and emit_frame -1 when T_b == 0 or no path is finite).  Returns -2 for U1 > 1024. */
long ea_ctc_viterbi_workspace_bytes(int B, int T, int Lmax);
int ea_ctc_viterbi_align(const void* x, long ld, int x_bf16, const int* targets, const int* in_len, const int* tgt_len,
                         void* workspace, int* tok_start, int* tok_end, int* frame_label, float* score, int B, int T, int V,
                         int Lmax, int blank, ea_stream_t stream);
long ea_rnnt_viterbi_workspace_bytes(int B, int T, int U1);
int ea_rnnt_viterbi_align(const float* lpb, const float* lpy, const int* logit_lengths, const int* target_lengths,
                          void* workspace, int* emit_frame, float* score, int B, int T, int U1, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Long-form forced alignment (csrc/align_long.hip): ea_ctc_viterbi_align's search for ONE sequence whose lattice does not fit a
 * workgroup -- a recording's stitched log-probs (ea_longform_stitch) against its whole transcript.  The reference has no forced
 * aligner of its own.  The lattice is cut into tiles of `frames` x `states` (ea_ctc_viterbi_long_tile); the tiles of one
 * anti-diagonal run in one launch, and launch boundaries are the only ordering between workgroups (no grid barrier, no
 * cooperative launch, no flag one workgroup waits on): ceil(T / frames) + ceil(S / states) + 1 launches per call, no device
 * allocation and no synchronisation inside.
 *
 * ea_ctc_viterbi_long_align: x fp32 or bf16 (x_bf16) [T][ld] log-probs (ld >= V), targets int32 [U] (may be NULL for U == 0),
 *   workspace: ea_ctc_viterbi_long_workspace_bytes(T, U) bytes, any contents (backpointers 2 bits per frame and state, the score
 *   vector alpha [S] and the tile edges [ceil(S / states)][T][2]).
 *   Lattice: blank y1 blank ... yU blank (S = 2U + 1 states); moves stay, +1, +2 (+2 only into a non-blank state whose label
 *   differs from the label two states earlier); frame 0 admits states 0 and 1, a path ends in state S-1 or S-2.
 *   TIE RULE: stay over +1 over +2; at the end S-1 over S-2.  Scores are fp32 sums in frame order: every output equals, BIT FOR
 *   BIT, what ea_ctc_viterbi_align gives for B = 1, in_len = T, tgt_len = Lmax = U wherever that call accepts the problem.
 *   Outputs (device): tok_start / tok_end int32 [U] = first frame of token u's non-blank run and one past its last frame;
 *   frame_label int32 [T] = u on a frame of token u, -1 on blank frames; frame_lp fp32 [T] = x[t][label of the chosen state]
 *   (their sum over a stretch of frames is that stretch's share of the score); score fp32 [1] (U == 0: the all-blank path;
 *   T == U == 0: 0).
 *   Infeasible (T < U + number of equal adjacent targets, or no finite path): score = -inf, tok_start = tok_end = -1,
 *   frame_label = -2, frame_lp = 0.  A target id outside [0, V) or equal to blank: score = NaN and the same fill, not aligned.
 *   Returns -2 for T < 0, U < 0, V < 1, blank outside [0, V), ld < V, T > 2^30 or U > 2^28 (ea_ctc_viterbi_long_workspace_bytes
 *   returns 0 for such T, U). */
int ea_ctc_viterbi_long_tile(int* frames, int* states);
long ea_ctc_viterbi_long_workspace_bytes(long T, long U);
int ea_ctc_viterbi_long_align(const void* x, long ld, int x_bf16, const int* targets, void* workspace, int* tok_start, int* tok_end,
                              int* frame_label, float* frame_lp, float* score, long T, int V, long U, int blank,
                              ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-token posteriors of a given label sequence (csrc/prefix_posterior.hip): the sum-product twins of the two aligners.  The
 * reference has them for attention-decoder hypotheses only (positional_scores); CTC and transducer hypotheses get them here.
 *   Psi_i = log P(the model's output starts with y1 .. yi | x), summed over all continuations and all alignments (Psi_0 = 0);
 *   log c_i = Psi_i - Psi_{i-1}: the posterior of token i given the audio and the tokens before it;
 *   log c_end = total - Psi_U, and sum_i log c_i + log c_end = total = log P(y | x) = -(CTC / RNN-T loss).
 * One workgroup per hypothesis, no workspace, outputs stay on the device (no host synchronisation).
 * Outputs of both: logc fp32 [N][Lmax + 1] (ea_rnnt_...: [B][U1]): position i < U holds log c_{i+1}, position U holds log c_end,
 *   positions past U hold 0; total fp32 [N]; psi fp32 [N][Lmax] ([B][U1 - 1]) or NULL: position i < U holds Psi_{i+1}, 0 past U.
 *   Every logc entry is clamped to <= 0.  Zero probability or an infeasible hypothesis: from the first i with Psi_i = -inf on,
 *   every factor and total are -inf, never NaN.
 *
 * ea_ctc_prefix_posteriors: x fp32 or bf16 (x_bf16) [B][T][ld] log-probs (ld >= V), targets int32 [N][Lmax], tgt_len int32 [N]
 *   (clamped to Lmax), utt int32 [N]: the row of x and in_len that hypothesis n reads (an n-best list shares its utterance's
 *   log-probs), in_len int32 [B] (clamped to T).  Lattice and move rules of ea_ctc_loss / ea_ctc_viterbi_align, log-add-exp for
 *   max; Psi_i = log sum_t x_t(y_i) * (alpha_{t-1}(blank before y_i) + [y_i != y_{i-1}] * alpha_{t-1}(y_{i-1})), the mass that
 *   ENTERS token i's state at frame t (at t = 0 only token 1, with x_0(y_1)); total = lse(alpha_T(S-1), alpha_T(S-2)).
 *   in_len == U == 0: total 0.  A target id outside [0, V) or equal to blank, or utt[n] outside [0, B): that hypothesis's
 *   outputs are NaN.  Returns -2 for Lmax > 1023, Lmax < 1, ld < V or blank outside [0, V).
 * ea_rnnt_prefix_posteriors: lpb / lpy fp32 [B][T][U1] as in ea_rnnt_scan, one lattice per hypothesis; logit_lengths /
 *   target_lengths int32 [B].  Psi_{u+1} = lse_{t < T_b} (alpha(t,u) + lpy(t,u)); total = alpha(T_b-1, U_b) + lpb(T_b-1, U_b)
 *   (= -loss of ea_rnnt_scan); T_b == 0: total and the factors 0 .. U_b are -inf.  Returns -2 for U1 > 1024 or T < 1. */
int ea_ctc_prefix_posteriors(const void* x, long ld, int x_bf16, const int* targets, const int* utt, const int* in_len,
                             const int* tgt_len, float* logc, float* total, float* psi, int N, int B, int T, int V, int Lmax,
                             int blank, ea_stream_t stream);
int ea_rnnt_prefix_posteriors(const float* lpb, const float* lpy, const int* logit_lengths, const int* target_lengths,
                              float* logc, float* total, float* psi, int B, int T, int U1, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-token posteriors of ONE label sequence of any length (csrc/prefix_posterior_long.hip): ea_ctc_prefix_posteriors'
 * quantities for a recording's stitched log-probs (ea_longform_stitch) against its whole transcript, the sum-product twin of
 * ea_ctc_viterbi_long_align.  Definitions, lattice, move rules and conventions are those of ea_ctc_prefix_posteriors, and both
 * kernels do the same fp32 operations in the same order (csrc/prefix_math.h).  The tiles are those of the long-form aligner
 * (ea_ctc_viterbi_long_tile); the tiles of one anti-diagonal run in one launch and launch boundaries are the only ordering
 * between workgroups: ceil(T / frames) + ceil(S / states) + 1 launches per call (2 for T == 0), no device allocation and no
 * synchronisation inside.  A tile whose first state no alignment reaches by its last frame computes nothing; every other tile
 * is computed (Psi counts prefixes whether or not they can still reach the end).
 *
 * ea_ctc_prefix_long_posteriors: x fp32 or bf16 (x_bf16) [T][ld] log-probs (ld >= V), targets int32 [U] (may be NULL for
 *   U == 0), workspace: ea_ctc_prefix_long_workspace_bytes(T, U) bytes, any contents (the score vector alpha [S], the tile edges
 *   [ceil(S / states)][T][2], the accumulators Psi [U] and 8 KiB of flags; no backpointers).
 *   Outputs (device): logc fp32 [U + 1]: position i < U holds log c_{i+1}, position U holds log c_end (U == 0: logc[0] = total,
 *   the all-blank path); total fp32 [1]; psi fp32 [U] or NULL: Psi_{i+1}.  Every logc entry is clamped to <= 0.  Zero probability
 *   or an infeasible sequence (T < U + number of equal adjacent targets): from the first i with Psi_i = -inf on every factor and
 *   total are -inf, never NaN.  T == 0: total = 0 for U == 0, else -inf.  A target id outside [0, V) or equal to blank: every
 *   output is NaN.
 *   Psi and total have the magnitude of the path score (thousands for an hour of audio) and carry fp32 rounding of that size;
 *   log c_i is the difference of two neighbours whose errors are strongly correlated; log c_end = total - Psi_U is not such a
 *   difference (DESIGN.md sections 3.10 and 8.6 have the figures).
 *   Returns -2 for T < 0, U < 0, V < 1, blank outside [0, V), ld < V, T > 2^30 or U > 2^28 (ea_ctc_prefix_long_workspace_bytes
 *   returns 0 for such T, U). */
long ea_ctc_prefix_long_workspace_bytes(long T, long U);
int ea_ctc_prefix_long_posteriors(const void* x, long ld, int x_bf16, const int* targets, void* workspace, float* logc,
                                  float* total, float* psi, long T, int V, long U, int blank, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Keyword spotting on CTC log-probs, offline and streamed (csrc/kws.hip): where a list of phrases is spoken, and how sure the
 * model is, from the per-frame log-probs alone -- no beam search, no transcript.  The reference has nothing of the kind.  The
 * (stream, keyword) pairs are independent; each is a max-plus scan over the frames with a free start frame, its state carried
 * across pieces in the stream's slot, so a stream fed in any pieces gives bit for bit the offline result.
 *
 * x: fp32 log-probs (the output of a log-softmax, finite) as rows [total_rows][ld], ld >= V.
 *   g_t = max_{v < V} x_t[v], the score of the greedy path at frame t;
 *   d_t(v) = x_t[v] - g_t, one fp32 subtraction: <= 0, and == 0 exactly on the frame's argmax.
 * A keyword is a token sequence y_1 .. y_L, 1 <= L <= 64, no blank among the tokens.  LATTICE: 2L - 1 states tok_1, blk_1,
 *   tok_2, ..., blk_{L-1}, tok_L -- no leading and no trailing blank, so a hit's bounds are tight.  Every state carries a pair
 *   (e, b): e (fp32) is the best sum of d over the paths that entered tok_1 at frame b and occupy the state now; (-inf, -1)
 *   means there is none.  Frames count from the stream's first frame.
 * FRAME UPDATE of state s, from the pairs before the frame.  Candidates, in this order: 1. stay (s); 2. step (s-1); 3. skip
 *   (s-2), only into a token state whose label differs from the token two states earlier; 4. for s == 0 only, a fresh start
 *   (0, t).  TIE RULE: the largest e, on a tie the first in that order.  If the chosen e is -inf the state becomes (-inf, -1),
 *   otherwise e' = e_chosen + d_t(label(s)) (one fp32 add; the label of a blk state is blank) and b' = b_chosen.  Every operation
 *   is a max, one add or one subtract and no reduction is re-associated: the result has exactly one set of fp32 bits.
 * DETECTION after the update of frame t, with tau_k = L_k * ln(theta_k) computed by the caller in fp32.  Per (stream, keyword):
 *   an open hit (or none), last_end (-1 at first), a hit list and its count.  If e(tok_L) >= tau_k and b(tok_L) > last_end there
 *   is a candidate (b, t, e): with no open hit it becomes the open hit; if b <= open.end it overlaps and replaces the open hit
 *   iff e >= open.e (a tie goes to the later end, so the hit covers the last token's whole run); otherwise the open hit is
 *   emitted and the candidate becomes the open hit.  Then, if there is an open hit and t - open.end > hold, it is emitted.  A
 *   candidate with b <= last_end is dropped.
 * EMIT appends (start, end, e) to the list if count < max_hits, increments count always (count > max_hits reports the overflow),
 *   sets last_end = open.end and leaves no open hit.  end is inclusive.
 * The confidence shown to users is exp(e / L): the geometric mean per token of p(keyword path) / p(greedy path), in (0, 1], and
 *   1 when the keyword's path is the greedy path.
 * A keyword is INACTIVE when its length is outside [1, Lmax] or it holds a token outside [0, V) or equal to blank: it never has a
 *   candidate (its state is not touched).
 *
 * State: max_streams * ea_ctc_kws_state_bytes(K, Lmax, max_hits) bytes, slot-major.  Per slot, int32 words: [0] frames consumed,
 *   [1] the stream frame of the first row of the slot's latest piece, then per keyword kw_words = 4 * Lmax + 6 + 3 * max_hits
 *   rounded up to even: e fp32 [2 * Lmax] (tok_{u+1} at 2u, blk_{u+1} at 2u + 1; blk_L and the states past L stay -inf), b int32
 *   [2 * Lmax], open.start (-1: no open hit), open.end, open.e (fp32), last_end, count, 0, then starts int32 [max_hits], ends
 *   int32 [max_hits], scores fp32 [max_hits].  ..._state_bytes returns 0 for K < 1, Lmax outside [1, 64] or max_hits < 1.
 * Conventions of ea_ctc_prefix_beam_stream_*: slots / slot_idx / n_new / row_off are device int32 [n]; a slot may be listed once
 *   per call; no call synchronises with the host; bad arguments return -2 and launch nothing; n <= 0 returns 0.
 * ..._reset: the listed slots get the state before frame 0; a slot outside [0, max_streams) is skipped.
 * ..._step: entry i runs the frames of rows row_off[i] .. row_off[i] + n_new[i] - 1 of x through every active keyword and
 *   advances its slot's frame counter by n_new[i].  It is skipped, its slot untouched, if its slot is out of range, if n_new[i]
 *   <= 0 or if a row of its piece lies outside [0, total_rows).  rowmax: caller-provided fp32 scratch [total_rows], receives g of
 *   every row of x.  kw_tokens int32 [K][Lmax], kw_len int32 [K], kw_tau fp32 [K], all on the device; hold >= 0 in frames.
 *   Two launches: the row maxima (one wave per row) with the entries' frame bookkeeping, then the scan, 256-thread workgroups,
 *   one keyword per wave, grid (ceil(K / 4), n).  The offline search is reset, one step over the whole utterances, then hits
 *   with flush: one per-frame body for both.
 * ..._hits: flush != 0 first emits the open hits of the listed slots (the audio's end).  Then the lists are copied into starts /
 *   ends int32 [n][K][max_hits] (-1 past the list), scores fp32 [n][K][max_hits] (0 past the list) and counts int32 [n][K].
 *   clear != 0 then empties the lists and zeroes the counts; the DP state, the open hits and last_end stay.  A slot out of range
 *   gets empty lists and count 0.
 * ea_ctc_kws_host: one utterance x_host [T][ld] on the host, flushed at the end, through the same __host__ __device__ update and
 *   detection functions as the kernel: its yardstick.  All arrays are host arrays; starts / ends / scores [K][max_hits], counts
 *   [K], filled as ..._hits fills them.  T == 0 gives empty lists. */
long ea_ctc_kws_state_bytes(int K, int Lmax, int max_hits);
int ea_ctc_kws_reset(void* state, const int* slots, int n, int max_streams, int K, int Lmax, int max_hits, ea_stream_t stream);
int ea_ctc_kws_step(const float* x, long ld, long total_rows, float* rowmax, const int* slot_idx, const int* n_new,
                    const int* row_off, int n, void* state, const int* kw_tokens, const int* kw_len, const float* kw_tau,
                    int max_streams, int K, int Lmax, int max_hits, int V, int blank, int hold, ea_stream_t stream);
int ea_ctc_kws_hits(void* state, const int* slots, int n, int flush, int clear, int max_streams, int K, int Lmax, int max_hits,
                    int* starts, int* ends, float* scores, int* counts, ea_stream_t stream);
int ea_ctc_kws_host(const float* x_host, long ld, int T, int V, const int* kw_tokens, const int* kw_len, const float* kw_tau, int K,
                    int Lmax, int blank, int hold, int max_hits, int* starts, int* ends, float* scores, int* counts);

/* ------------------------------------------------------------------------------------------
 * Long-form recognition for offline CTC models (csrc/long_form.hip): the join of the logits of one recording's overlapping
 * windows into one fp32 log-prob matrix on the recording's own frame axis.  The reference has no long-form path (its recognizer
 * takes a recording as one utterance), so these two entry points replace nothing of it; what they spare is a host loop of
 * slices, log-softmaxes and index copies per junction.
 *
 * logits: [Nw][Tw][ld >= V], bf16 (is_bf16 != 0) or fp32, as the encoder wrote them; counts int32 [Nw] (device): the frames of
 * each window, in [0, Tw]; window n holds global frames n * Hf + [0, counts[n]), 1 <= Hf <= Tw.
 * ea_longform_cuts: per junction n (windows n and n + 1, n < Nw - 1) the overlap is the global frames [lo, hi), lo = (n + 1) * Hf,
 *   hi = min(n * Hf + counts[n], lo + counts[n + 1]).  b(j) = min over the two windows of the log-softmax of frame j at column
 *   `blank` (the bits ea_log_softmax_* writes there).  A cut c gives the frames < c to window n and the frames >= c to window
 *   n + 1; the candidates are lo + edge <= c <= hi - edge, score(c) = min of b(j) over j in [c - guard, c + guard) within [lo, hi),
 *   or, that range being empty, b at the overlap frame nearest c (c, or hi - 1 for c == hi).  cuts[n] = the candidate with the
 *   largest score, ties to the smallest |2c - (lo + hi)|, then to the smallest c; without candidates floor((lo + hi) / 2);
 *   scores[n] = its score.  An empty overlap (hi <= lo) gives cuts[n] = lo, scores[n] = 0.  Nw == 1 launches nothing.
 *   Tw - Hf <= 12288 (the b(j) of an overlap live in LDS).
 * ea_longform_stitch: out fp32 [T][ldo >= V], T <= (Nw - 1) * Hf + Tw; row t = the log-softmax of frame t's row in the window
 *   that owns it under `cuts` (window 0 before cuts[0], window n from cuts[n - 1] up to cuts[n], the last window after), bit for
 *   bit what ea_log_softmax_* writes for that row; columns >= V of out are not written, rows of other windows are not read.
 *   Needs Tw < 2 * Hf for Nw > 1 (a frame lies in at most two windows, so the cuts increase).  cuts may be NULL for Nw == 1.
 *   A frame whose owner under `cuts` does not hold it is left unwritten.
 * Bad arguments return -2 and launch nothing. */
int ea_longform_cuts(const void* logits, int is_bf16, long ld, const int* counts, int Nw, int Tw, int V, int Hf, int blank, int edge,
                     int guard, int* cuts, float* scores, ea_stream_t stream);
int ea_longform_stitch(const void* logits, int is_bf16, long ld, const int* counts, const int* cuts, int Nw, int Tw, int V, int Hf,
                       long T, float* out, long ldo, ea_stream_t stream);
/* Long-form recognition for transducer models: the join of the windows' ENCODER OUTPUTS (`_x_bt`, not logits) into one [T][D]
 * matrix on the recording's own frame axis, which `joint_encoder_branch` and the frame-synchronous searches then read as one
 * utterance's.  There is no blank column to cut at: the cut goes where the two windows' encoders agree.
 *
 * x: [Nw][Tw][ld >= D], bf16 (is_bf16 != 0) or fp32; counts, Nw, Tw, Hf, the windows' frames and the overlap [lo, hi) of junction
 * n exactly as above.
 * ea_longform_feature_cuts: for overlap frame j, a = window n's row of it (row j - n * Hf) and b = window n + 1's (row j - lo),
 *   columns < D; num = sum_k (a_k - b_k)^2, den = sum_k a_k^2 + sum_k b_k^2, both accumulated in fp32; d(j) = num / den if den > 0,
 *   else 0, so 0 <= d <= 2 and 0 means identical rows.  s(j) = -d(j) takes the place of b(j); everything after it is the rule of
 *   ea_longform_cuts unchanged: score(c) = min of s over [c - guard, c + guard) within [lo, hi) with the same fallback for an
 *   empty range, candidates lo + edge <= c <= hi - edge, the order (score descending, |2c - (lo + hi)|, c), floor((lo + hi) / 2)
 *   without candidates, cuts[n] = lo and scores[n] = 0 for an empty overlap.  Scores are <= 0; 0: both windows give the same
 *   features around the cut.  Nw == 1 launches nothing.  Tw - Hf <= 12288.  Rows >= counts[n] and columns >= D are never read.
 *   The order in which a sum's terms are added is not part of the rule; each sum is within (D + 3) * 2^-24 of exact, relatively.
 * ea_longform_stitch_rows: out [T][ldo >= D] of the same element type, elem_bytes = 2 or 4; row t = the bit copy of the D
 *   elements of frame t's row in the window that owns it under `cuts` (the owner rule of ea_longform_stitch); columns >= D of
 *   out are not written, rows of other windows are not read.  T <= (Nw - 1) * Hf + Tw and T <= INT_MAX; Tw < 2 * Hf for Nw > 1;
 *   cuts may be NULL for Nw == 1; a frame whose owner under `cuts` does not hold it is left unwritten.
 * Bad arguments return -2 and launch nothing. */
int ea_longform_feature_cuts(const void* x, int is_bf16, long ld, const int* counts, int Nw, int Tw, int D, int Hf, int edge, int guard,
                             int* cuts, float* scores, ea_stream_t stream);
int ea_longform_stitch_rows(const void* x, int elem_bytes, long ld, const int* counts, const int* cuts, int Nw, int Tw, int D, int Hf,
                            long T, void* out, long ldo, ea_stream_t stream);
/* Joint network element-wise stages (espresso/models/transformer/speech_transformer_transducer_base.py:276-299):
 * Z[b][t][u] = relu(E[b][t] + D[b][u]) (bf16, E [B*T][J], D [B*U1][J], Z [B*T*U1][J], J % 8 == 0) and its backward
 * reductions dE[b][t] = sum_u dZ[b][t][u], dD[b][u] = sum_t dZ[b][t][u] (either output may be NULL). */
int ea_joint_add_relu(const void* E, const void* D, void* Z, int B, int T, int U1, int J, ea_stream_t stream);
int ea_joint_reduce(const void* dZ, void* dE, void* dD, int B, int T, int U1, int J, ea_stream_t stream);
/* The training path's form (round 6): E and D are the fp32 LayerNorm outputs (ea_layernorm_fwd_f32out), the sum and the ReLU are
 * evaluated in fp32 as in the reference's autocast run (:292-294) and only Z — fc_out's bf16 GEMM operand — is rounded; dE / dD
 * leave as fp32 sums (inputs of ea_layernorm_bwd_f32dy).  relu'(E + D) is recovered from Z > 0, which is exact for the fp32 sum. */
int ea_joint_add_relu_f32(const float* E, const float* D, void* Z, int B, int T, int U1, int J, ea_stream_t stream);
int ea_joint_reduce_f32(const void* dZ, float* dE, float* dD, int B, int T, int U1, int J, ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Chunk-streaming encoder attention (csrc/stream_attention.hip): incremental inference of encoders trained with
 * `encoder.chunk_size = cs > 0`, `chunk_left_window = L`, `chunk_right_window = 0` — the visibility of
 * espresso/tools/utils.py chunk_streaming_mask(always_partial_in_last=True), one chunk at a time for many streams.
 *   cache   : one layer's ring, bf16 [max_streams][W][2C], W = (L+1)*cs slots, K in columns [0,C), V in [C,2C); chunk c of a
 *             stream occupies slots (c % (L+1))*cs .. +cs.
 *   frames  : int [max_streams], device: frames appended to a stream before the chunk in flight (a multiple of cs; the
 *             host never reads it).  The chunk index, the validity of every slot and its absolute position follow from it.
 *   slot_idx, n_new, row_off : int [B]: batch entry b is stream slot_idx[b] with n_new[b] <= cs new rows at rows
 *             row_off[b] .. of the packed [total_rows][*] activations.  n_new[b] == 0: idle, nothing read or written.
 *             Entries with out-of-range values are skipped.
 * ea_stream_kv_append : ring <- the 2C contiguous bf16 (k, v) of rows row_off[b]+i of `kv` (ldkv elements per row).
 * ea_stream_attention : out[row_off[b]+i][h*dh+d] = softmax_j(qu_i . k_j + qv_i . pp[pp_center + pos_j - pos_i]) v_j over the
 *             valid slots j (previous <= L chunks + the n_new[b] rows of the current one; append first).  qu / qv bf16
 *             [total_rows][ldq] from ea_relpos_q_prep (pre-scaled); pp bf16 [pp_rows][ldpp] projected relative table, row
 *             pp_center <-> distance 0, rows pp_center-(W-1) .. pp_center+cs-1 are read; pp == NULL: plain attention (qv
 *             ignored).  fp32 softmax; P is normalised, then rounded to bf16 before P.V (ea_relpos_softmax_fwd's rounding).
 * ea_stream_advance   : frames[slot_idx[b]] += n_new[b], once per chunk after the last layer.
 * ea_stream_attention_supported: dh in {16, 32, 64}, cs <= 128, (L+1)*cs <= 512, C % dh == 0, C % 8 == 0; the launchers
 *             return -2 otherwise. */
int ea_stream_attention_supported(int dh, int chunk_size, int left_chunks, int C);
int ea_stream_kv_append(const void* kv, long ldkv, void* cache, const int* slot_idx, const int* n_new, const int* row_off,
                        const int* frames, int B, int C, int chunk_size, int left_chunks, int max_streams, int total_rows,
                        ea_stream_t stream);
int ea_stream_attention(const void* qu, const void* qv, long ldq, const void* cache, const void* pp, long ldpp, int pp_center,
                        int pp_rows, const int* slot_idx, const int* n_new, const int* row_off, const int* frames, void* out,
                        long ldo, int B, int H, int dh, int chunk_size, int left_chunks, int max_streams, int total_rows,
                        ea_stream_t stream);
int ea_stream_advance(int* frames, const int* slot_idx, const int* n_new, int B, int chunk_size, int max_streams,
                      ea_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Streamed causal Conformer convolution module (csrc/stream_convmodule.hip): GLU -> causal depthwise conv -> BatchNorm1d
 * (running statistics) -> SiLU for the new rows of every stream that has a chunk ready, with the same meta rows as
 * ea_stream_attention.
 *   Y         : bf16 [total_rows][2C], pointwise_conv1 output of the new rows.
 *   w         : fp32 [C][KW];  mean_rstd : fp32 [2][C] from ea_bn_from_running;  gamma, beta : fp32 [C].
 *   carry     : one layer's state, bf16 [max_streams][KW-1][C]: the last KW-1 rows of U = bf16(a * sigmoid(g)) of each stream,
 *               oldest first.  A zeroed slab is the utterance's left zero padding.
 * For an entry with 0 < n = n_new[b] <= chunk_size, a slot in range and rows inside the buffer: X = [carry[slot] ; U_new]
 * (KW-1+n rows), Z[j] = bf16(sum_k w[k] * X[j+k]) (taps ascending, fp32), H[j] = bf16(silu(Z[j]*sc + sh)) with sc = rstd*gamma,
 * sh = beta - mean*sc (ea_bn_act_fwd's arithmetic), then carry[slot] <- the last KW-1 rows of X.  Any other entry is skipped:
 * nothing of it is read or written.  H, Z : bf16 [total_rows][C]; Z (the pre-BatchNorm value) may be NULL.
 * ea_stream_convmodule_supported: C % 8 == 0, KW in {3,7,15,31}, chunk_size <= 128; the launcher returns -2 otherwise. */
int ea_stream_convmodule_supported(int C, int KW, int chunk_size);
int ea_stream_glu_dwconv_bn_act(const void* Y, const float* w, const float* mean_rstd, const float* gamma, const float* beta,
                                void* carry, const int* slot_idx, const int* n_new, const int* row_off, void* H, void* Z, int B,
                                int C, int KW, int chunk_size, int max_streams, int total_rows, ea_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ESPRESSO_AMD_H */
