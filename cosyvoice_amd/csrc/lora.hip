// Per-sequence LoRA for the speech LM (include/cosyvoice_amd_lora.h): shrink u = x A_a^T and expand y (+)= s_a u B_a^T, each row with the
// adapter of its own sequence.  Bandwidth-bound gather-GEMVs: 16-byte loads of the 16-bit operands, fp32 accumulation in an order fixed
// by (K, r) alone, no exchange between rows or workgroups.  Rows that share an adapter re-read its A / B out of L2.
#include "cv_device.h"
#include "../../include/cosyvoice_amd_lora.h"

namespace {

constexpr int SHRINK_WAVES = 4;    // waves per workgroup
constexpr int SHRINK_JW = 4;       // u columns per wave: the x chunk of a lane is loaded once for all of them
constexpr int SHRINK_JB = SHRINK_WAVES * SHRINK_JW;
constexpr int EXPAND_THREADS = 256;
constexpr int MAX_R_TOT = 96;

__host__ __device__ inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <int DT>
__device__ __forceinline__ void unpack8(const uint4& v, float (&f)[8]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = Elem16<DT>::to_f32((uint16_t)(w[i] & 0xFFFFu));
    f[2 * i + 1] = Elem16<DT>::to_f32((uint16_t)(w[i] >> 16));
  }
}

// grid (ceil(R_tot / 16), rows), 256 threads: wave w owns columns j0 + 4w .. j0 + 4w + 3 of one row
template <int DT>
__global__ __launch_bounds__(SHRINK_WAVES * 64) void lora_shrink_kernel(const cv_lora_shrink_params p) {
  const int row = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * SHRINK_JB + wave * SHRINK_JW;
  if (j0 >= p.R_tot) return;                                   // wave-uniform; R_tot % 8 == 0, so a live wave owns four columns
  const int a = p.row_adapter[row / p.rows_per_seq];
  float* u = p.u + (size_t)row * p.ldu + j0;
  if (a < 0 || a >= p.n_slots) {                                // base model only (a slot past the bank is treated the same: never read)
    if (lane < SHRINK_JW) u[lane] = 0.0f;
    return;
  }
  const uint16_t* x = (const uint16_t*)p.x + (size_t)row * p.ldx;
  const uint16_t* A = (const uint16_t*)p.A + ((size_t)a * p.R_tot + j0) * p.K;
  float acc[SHRINK_JW] = {0.0f, 0.0f, 0.0f, 0.0f};
  const int nchunk = p.K >> 3;
  for (int c = lane; c < nchunk; c += 64) {
    float xf[8];
    unpack8<DT>(*(const uint4*)(x + 8 * c), xf);
#pragma unroll
    for (int jj = 0; jj < SHRINK_JW; ++jj) {
      float af[8];
      unpack8<DT>(*(const uint4*)(A + (size_t)jj * p.K + 8 * c), af);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[jj] = fmaf(af[e], xf[e], acc[jj]);
    }
  }
#pragma unroll
  for (int jj = 0; jj < SHRINK_JW; ++jj) acc[jj] = wave_sum(acc[jj]);
  if (lane < SHRINK_JW) u[lane] = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
}

template <int DT, int R>
__device__ __forceinline__ float expand_dot(const uint16_t* __restrict__ b, const float* __restrict__ u) {
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < R / 8; ++c) {
    float bf[8];
    unpack8<DT>(*(const uint4*)(b + 8 * c), bf);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(bf[e], u[8 * c + e], acc);
  }
  return acc;
}

// grid (ceil(cols / 256), rows): one thread per output column (SWIGLU: per h column, which owns one gate and one up column)
template <int DT, int R>
__global__ __launch_bounds__(EXPAND_THREADS) void lora_expand_kernel(const cv_lora_expand_params p) {
  __shared__ float us[MAX_R_TOT];
  const int row = blockIdx.y;
  const int a_raw = p.row_adapter[row / p.rows_per_seq];
  const int a = (a_raw < 0 || a_raw >= p.n_slots) ? -1 : a_raw;
  const int n = blockIdx.x * EXPAND_THREADS + threadIdx.x;
  if (p.mode == CV_LORA_ADD && a < 0) return;                   // block-uniform
  float s = 0.0f;
  if (a >= 0) {
    // the u values this block needs: every segment's r columns (at most 3 r <= 96)
    const float* urow = p.u + (size_t)row * p.ldu;
    for (int i = threadIdx.x; i < p.n_seg * R; i += EXPAND_THREADS) us[i] = urow[p.seg[i / R].u_off + i % R];
    s = p.s[a];
  }
  __syncthreads();
  const uint16_t* B = (const uint16_t*)p.B + (a >= 0 ? (size_t)a * p.N * R : 0);
  if (p.mode == CV_LORA_SWIGLU) {
    const int I = p.N >> 1;
    if (n >= I) return;
    const float* y = p.y + (size_t)row * p.ldy + 32 * (n >> 4) + (n & 15);
    float g = y[0], up = y[16];
    if (a >= 0) {
      g += s * expand_dot<DT, R>(B + (size_t)n * R, us);
      up += s * expand_dot<DT, R>(B + (size_t)(I + n) * R, us + R);
    }
    ((uint16_t*)p.h)[(size_t)row * p.ldh + n] = Elem16<DT>::from_f32(act_silu(g) * up);
    return;
  }
  if (n >= p.N) return;
  float* y = p.y + (size_t)row * p.ldy + n;
  if (a < 0) { *y = 0.0f; return; }                             // STORE of a base-only row
  const int sg = (p.n_seg > 2 && n >= p.seg[2].n_begin) ? 2 : (p.n_seg > 1 && n >= p.seg[1].n_begin) ? 1 : 0;
  const float d = s * expand_dot<DT, R>(B + (size_t)n * R, us + sg * R);
  *y = p.mode == CV_LORA_STORE ? d : *y + d;
}

}  // namespace

extern "C" int cv_sizeof_lora_shrink_params(void) { return (int)sizeof(cv_lora_shrink_params); }
extern "C" int cv_sizeof_lora_expand_params(void) { return (int)sizeof(cv_lora_expand_params); }

extern "C" int cv_lora_shrink(const cv_lora_shrink_params* pp, void* stream) {
  if (!pp) return CV_ERR_ARG;
  const cv_lora_shrink_params& p = *pp;
  if (p.rows <= 0 || p.rows_per_seq <= 0 || p.K <= 0 || p.R_tot <= 0 || p.n_slots <= 0) return CV_ERR_ARG;
  if (!p.x || !p.A || !p.row_adapter || !p.u) return CV_ERR_ARG;
  if (p.dtype != CV_BF16 && p.dtype != CV_F16) return CV_ERR_UNSUPPORTED;
  if ((p.K & 31) || (p.R_tot & 7) || p.R_tot > MAX_R_TOT) return CV_ERR_UNSUPPORTED;
  if (p.ldx < p.K || (p.ldx & 7) || p.ldu < p.R_tot) return CV_ERR_ARG;
  if (!aligned_to(p.x, 16) || !aligned_to(p.A, 16) || !aligned_to(p.row_adapter, 4) || !aligned_to(p.u, 4)) return CV_ERR_ARG;
  if (p.rows > 65535) return CV_ERR_UNSUPPORTED;               // grid.y
  const dim3 grid((p.R_tot + SHRINK_JB - 1) / SHRINK_JB, p.rows);
  with_dt16(p.dtype, [&](auto DT) { hipLaunchKernelGGL(lora_shrink_kernel<DT()>, grid, dim3(SHRINK_WAVES * 64), 0, (hipStream_t)stream, p); });
  CV_CHECK_LAUNCH();
  return CV_OK;
}

extern "C" int cv_lora_expand(const cv_lora_expand_params* pp, void* stream) {
  if (!pp) return CV_ERR_ARG;
  const cv_lora_expand_params& p = *pp;
  if (p.rows <= 0 || p.rows_per_seq <= 0 || p.N <= 0 || p.n_slots <= 0) return CV_ERR_ARG;
  if (p.n_seg < 1 || p.n_seg > 3) return CV_ERR_ARG;
  if (p.mode != CV_LORA_ADD && p.mode != CV_LORA_STORE && p.mode != CV_LORA_SWIGLU) return CV_ERR_ARG;
  if (!p.u || !p.B || !p.s || !p.row_adapter || !p.y) return CV_ERR_ARG;
  if (p.dtype != CV_BF16 && p.dtype != CV_F16) return CV_ERR_UNSUPPORTED;
  if (p.r != 8 && p.r != 16 && p.r != 32) return CV_ERR_UNSUPPORTED;
  int next = 0;
  for (int i = 0; i < p.n_seg; ++i) {                           // ascending, disjoint, covering [0, N); u columns inside the row
    const cv_lora_segment& sg = p.seg[i];
    if (sg.n_begin != next || sg.n_end <= sg.n_begin || sg.u_off < 0 || sg.u_off + p.r > p.ldu) return CV_ERR_ARG;
    next = sg.n_end;
  }
  if (next != p.N) return CV_ERR_ARG;
  if (!aligned_to(p.u, 4) || !aligned_to(p.B, 16) || !aligned_to(p.s, 4) || !aligned_to(p.row_adapter, 4) || !aligned_to(p.y, 4))
    return CV_ERR_ARG;
  int cols = p.N;
  if (p.mode == CV_LORA_SWIGLU) {
    const int I = p.N >> 1;
    if ((p.N & 31) || p.n_seg != 2 || p.seg[0].n_end != I) return CV_ERR_UNSUPPORTED;
    if (!p.h || !aligned_to(p.h, 2) || p.ldh < I || p.ldy < p.N) return CV_ERR_ARG;
    cols = I;
  } else if (p.ldy < p.N) {
    return CV_ERR_ARG;
  }
  if (p.rows > 65535) return CV_ERR_UNSUPPORTED;               // grid.y
  const dim3 grid((cols + EXPAND_THREADS - 1) / EXPAND_THREADS, p.rows);
  with_dt16(p.dtype, [&](auto DT) {
    with_value<8, 16, 32>(p.r, [&](auto R) {
      hipLaunchKernelGGL((lora_expand_kernel<DT(), R()>), grid, dim3(EXPAND_THREADS), 0, (hipStream_t)stream, p);
    });
  });
  CV_CHECK_LAUNCH();
  return CV_OK;
}
