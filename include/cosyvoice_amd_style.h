/* cosyvoice_amd — C ABI of the speaker-encoder-v2 kernels (csrc/style.hip), exported by the same libcosyvoice_amd.so.
 *
 * SpeakerEmbedding (cosyvoice/speaker/speaker_encoder.py:119-270) = CAM++ timbre vector (cosyvoice_amd.h, cv_spk_*) + a style
 * vector: linear spectrogram -> PosteriorEncoder (posterior_encoder.py:6-37; WN, modules.py:145-219) -> StyleEncoder_v2
 * (style_encoder.py:21-114; Conv1dGLU modules.py:498-515, MultiHeadAttention :551-606) -> GlobalStyleTokens_v2
 * (style_encoder.py:117-157; MultiHeadAttention_GivenK modules.py:666-713) -> StyleFuser "Add" (style_encoder.py:160-184).
 * The 1x1 convs and Linears of that chain are cv_gemm calls; the entry points here are what cv_gemm cannot express.
 *
 * Conventions as in cosyvoice_amd.h: cv_status return codes, device pointers, a hipStream_t as `void* stream`, arguments
 * checked before anything is launched.  All tensors fp32, channels-last [B][T][ld], ragged through a DEVICE int32 len[B]
 * (clamped to [0, T]): rows at or past len[b] read as zero whatever the buffer holds and are written as zero.  All products are
 * the exact-f32 MFMA (v_mfma_f32_16x16x4_f32); no atomics; every output element's summation order is fixed by its own indices,
 * so a batch row is bit-identical to that sequence run alone.
 */
#ifndef COSYVOICE_AMD_STYLE_H
#define COSYVOICE_AMD_STYLE_H
#include "cosyvoice_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One WaveNet layer of WN (modules.py:197-218, gin_channels = 0, dilation 1) in one launch, 32 rows of one sequence per workgroup:
 *   a    = conv_k5(x) + b_in                       [T][2C]   implicit GEMM, K = 5C, k = tap * C + ci, padding 2
 *   g    = tanh(a[:, :C]) * sigmoid(a[:, C:])      [32][C]   stays in LDS (commons.py:106-112)
 *   rs   = g w_rs^T + b_rs                         [T][n_rs]
 *   n_rs == 2C:  x_out = x + rs[:, :C];  skip (+)= rs[:, C:]          n_rs == C (the last layer):  skip (+)= rs
 * skip_init != 0 writes skip = ... instead of accumulating (the first layer: `output = zeros_like(x)`).  x_out must not alias x
 * (a tile reads a 2-row halo of its neighbours).  Weight norm is folded by the caller.  C = 512, taps = 5 are what is built:
 * other values return CV_ERR_UNSUPPORTED. */
typedef struct cv_wn_layer_params {
  int32_t B, T, C, taps;
  const int32_t* len;                              /* [B] */
  const float* x; int64_t x_bs; int32_t ldx;       /* [B][T][C] */
  const float* w_in; const float* b_in;            /* [2C][taps * C], [2C] */
  const float* w_rs; const float* b_rs;            /* [n_rs][C], [n_rs] */
  int32_t n_rs, skip_init;
  float* x_out; int64_t xo_bs; int32_t ldxo;       /* [B][T][C]; unused (may be NULL) when n_rs == C */
  float* skip; int64_t skip_bs; int32_t ldskip;    /* [B][T][C] */
} cv_wn_layer_params;
int cv_sizeof_wn_layer_params(void);
int cv_wn_layer(const cv_wn_layer_params* p, void* stream);

/* The gate of that layer alone (commons.py:106-112), for the layer composed from cv_gemm launches (the conv, this, the 1x1) that
 * tools/style_bench.py times against cv_wn_layer: a [rows][lda] = [tanh half (C) | sigmoid half (C)] -> g [rows][ldg] = tanh * sigmoid. */
int cv_wn_gate(const float* a, int32_t lda, float* g, int32_t ldg, int32_t rows, int32_t C, void* stream);

/* Conv1dGLU (modules.py:498-515) in one launch: a = conv_k5(x) + bias [T][2C]; y = x + a[:, :C] * sigmoid(a[:, C:]).
 * C = 256, taps = 5 are what is built.  y must not alias x. */
typedef struct cv_glu_conv_params {
  int32_t B, T, C, taps;
  const int32_t* len;
  const float* x; int64_t x_bs; int32_t ldx;
  const float* w; const float* bias;               /* [2C][taps * C] with k = tap * C + ci, [2C] */
  float* y; int64_t y_bs; int32_t ldy;
} cv_glu_conv_params;
int cv_sizeof_glu_conv_params(void);
int cv_glu_conv(const cv_glu_conv_params* p, void* stream);

/* MultiHeadAttention_GivenK (modules.py:689-710) for one query row per sequence: q [B][ldq] (W_query already applied) against
 * n_tok keys / values that depend on weights only, k, v [H][n_tok][64] (head-major, computed once at load):
 * out[b][h * 64 + d] = softmax_t(q_h . k_h[t] * scale) . v_h[:, d].  fp32 softmax; one workgroup per (head, sequence). */
int cv_gst_attention(const float* q, int32_t ldq, const float* k, const float* v, float* out, int32_t ldo, int32_t B, int32_t H,
                     int32_t n_tok, float scale, void* stream);

/* Self-attention of the style encoder (modules.py:577-630) in fp32: heads of 64 packed inside a row, q / k / v [B][T][ld] (any
 * column offset folded into the pointers), keys t >= len[b] masked, out[b][t][h * 64 + d]; query rows t >= len[b] are written 0.
 * The 16 x T score block of a workgroup lives in LDS: T <= 2400 (30 s of 80 frames/s), else CV_ERR_UNSUPPORTED. */
int cv_style_attention(const float* q, const float* k, const float* v, int64_t qkv_bs, int32_t ld, float* out, int64_t o_bs, int32_t ldo,
                       const int32_t* len, int32_t B, int32_t T, int32_t H, float scale, void* stream);

/* posterior_encoder.py:35-36: stats [B][T][ld_stats] = [m (C) | logs (C)], noise [B][T][C] -> z [B][T][ldz] = m + noise * exp(logs). */
int cv_posterior_sample(const float* stats, int32_t ld_stats, const float* noise, float* z, int32_t ldz, const int32_t* len, int32_t B,
                        int32_t T, int32_t C, void* stream);

/* StyleEncoder_v2.temporal_avg_pool (style_encoder.py:73-81): out[b][c] = sum_{t < len[b]} x[b][t][c] / len[b] (0 when len[b] = 0).
 * Four row phases per channel, summed in phase order.  C % 64 == 0. */
int cv_masked_mean(const float* x, int64_t x_bs, int32_t ldx, const int32_t* len, int32_t B, int32_t T, int32_t C, float* out,
                   int32_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif
