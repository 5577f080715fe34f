/* cosyvoice_amd — C ABI of the per-sequence LoRA kernels (csrc/lora.hip), exported by the same libcosyvoice_amd.so.
 *
 * The fork ships voices as a base model plus per-speaker low-rank adapters (cosyvoice/loralib/layers.py:222-235, unmerged form):
 *   Linear     y = x W^T + b + s (x A^T) B^T        A (r, in), B (out, r), s = lora_alpha / r (1 with "noscale")
 *   Embedding  e = W[idx] + s (A^T[idx]) B^T        A (r, vocab), B (dim, r)
 * The base product stays with the kernels of cosyvoice_amd.h; the two entry points here add the low-rank term per ROW, each row with
 * the adapter of its own sequence, so one weight stream serves a batch of different voices.
 *
 * Conventions as in cosyvoice_amd.h: cv_status return codes, device pointers, a hipStream_t as `void* stream`, arguments checked
 * before anything is launched.  Adapters live in BANKS of n_slots equally shaped 16-bit matrices; the adapter of a row is
 *   a = row_adapter[row / rows_per_seq]            (DEVICE int32; rows_per_seq as in cv_rope_append: 1 = decode, Lp = prefill)
 * and a < 0 means "base model only" (the reference's infer_base_model = True).  A slot no row names is never read.
 * Supported: r in {8, 16, 32}, K % 32 == 0, any N >= 1, rows >= 1; anything else is CV_ERR_UNSUPPORTED before a launch.  Null or
 * misaligned pointers (16 bytes for x, A, B; 4 for the rest), pitches smaller than the extent, a slot count < 1: CV_ERR_ARG.
 *
 * Arithmetic: fp32 accumulation, no atomics, nothing device-wide.  The summation order of an output element depends on (K, r)
 * only: a row's result is BIT-IDENTICAL whatever `rows` is, whichever launch position the row has and whatever the other rows'
 * adapters are.
 *   shrink: lane l of a wave sums the 8-element chunks l, l + 64, l + 128, ... of the K products in ascending k, then the 64 lane
 *           sums are combined by the xor butterfly 32, 16, 8, 4, 2, 1.
 *   expand: one thread per output column, j = 0 .. r-1 in ascending order, then one multiply by s_a and one add.
 * Neither kernel writes outside [0, rows) x [0, N); u is written only in [0, rows) x [0, R_tot).
 */
#ifndef COSYVOICE_AMD_LORA_H
#define COSYVOICE_AMD_LORA_H
#include "cosyvoice_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* u[row][j] = sum_k A_a[j][k] * x[row][k], j < R_tot;  a < 0: u[row][:] = 0.
 * The A matrices of all projections that read the same input are stacked along j (q|k|v: R_tot = 3r, gate|up: 2r), so R_tot is any
 * multiple of 8 up to 96.  u is fp32 and is never rounded to 16 bits. */
typedef struct cv_lora_shrink_params {
  int32_t dtype;                                   /* CV_BF16 / CV_F16: x and A */
  int32_t rows, rows_per_seq, K, R_tot, n_slots;
  const void* x; int32_t ldx;                      /* 16-bit [rows][ldx], ldx % 8 == 0 */
  const void* A;                                   /* 16-bit bank [n_slots][R_tot][K] */
  const int32_t* row_adapter;                      /* [ceil(rows / rows_per_seq)] */
  float* u; int32_t ldu;                           /* fp32 [rows][ldu] */
} cv_lora_shrink_params;
int cv_sizeof_lora_shrink_params(void);
int cv_lora_shrink(const cv_lora_shrink_params* p, void* stream);

/* Column segment of an expand: columns [n_begin, n_end) read u[row][u_off .. u_off + r).  Segments are ascending, disjoint and
 * cover [0, N) exactly (q|k|v of one layer is ONE launch with three segments). */
typedef struct cv_lora_segment { int32_t n_begin, n_end, u_off; } cv_lora_segment;

enum { CV_LORA_ADD = 0, CV_LORA_STORE = 1, CV_LORA_SWIGLU = 2 };

/* d[row][n] = s_a * sum_{j<r} B_a[n][j] * u[row][u_off(n) + j]
 *   CV_LORA_ADD     y[row][n] += d          fp32 y [rows][ldy]; rows with a < 0 are left bit-unchanged (not read, not written).
 *                   The qkv buffer before RoPE, the residual after o_proj, the logits, embedding rows.
 *   CV_LORA_STORE   y[row][n]  = d          fp32; rows with a < 0 store zeros.  The extra split-K slab after down_proj, which the
 *                   following cv_rmsnorm_reduce sums with nslab = ksplit + 1.
 *   CV_LORA_SWIGLU  N = 2I, B rows [0, I) = gate, [I, 2I) = up, exactly two segments {0, I, .}, {I, 2I, .}, I % 16 == 0.
 *                   y holds the fp32 gate / up PRE-ACTIVATIONS in 16-column blocks [gate16 | up16] (column c of gate at
 *                   32 (c / 16) + c % 16, of up 16 further), the order in which mode-0 cv_skinny_gemm over an interleave-packed
 *                   weight and cv_gemm over the interleaved prefill weight leave them.  Writes
 *                   h[row][c] = silu(g + d_gate) * (up + d_up) as 16-bit [rows][ldh], c < I; rows with a < 0 get silu(g) * up.
 *                   y is only read. */
typedef struct cv_lora_expand_params {
  int32_t dtype;                                   /* CV_BF16 / CV_F16: B and h */
  int32_t rows, rows_per_seq, N, r, n_slots, mode, n_seg;
  cv_lora_segment seg[3];
  const float* u; int32_t ldu;                     /* fp32 [rows][ldu] */
  const void* B;                                   /* 16-bit bank [n_slots][N][r] */
  const float* s;                                  /* fp32 [n_slots] */
  const int32_t* row_adapter;
  float* y; int32_t ldy;                           /* fp32 [rows][ldy] */
  void* h; int32_t ldh;                            /* CV_LORA_SWIGLU only: 16-bit [rows][ldh] */
} cv_lora_expand_params;
int cv_sizeof_lora_expand_params(void);
int cv_lora_expand(const cv_lora_expand_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif
