// Speaker embedding: the Kaldi fbank + CMN of CosyVoiceFrontEnd._extract_spk_embedding
// (cosyvoice/cli/frontend.py:91-100) and the CAM++ x-vector network it feeds (cosyvoice/speaker/CAMPPlus.py:214-451).
// The fbank's DFT and mel projection run on cv_gemm; the kernels here are the power spectrum and log + CMN between and
// after them, one MFMA convolution that covers every Conv2d / Conv1d of the network, the CAM context gate and the
// statistics pooling.
//
// Ragged batches: every kernel takes per-sequence lengths on the device and reads / reduces over a sequence's own rows only;
// rows at and past a length are written as zeros.  No reduction depends on the padded length or on the other sequences, and
// none uses atomics, so each row of a batch is bit-identical to that sequence run alone.
#include <float.h>
#include "cv_device.h"

namespace {

// spec [rows][ld_spec] = [re(0..nbins) | im(0..nbins)]  ->  pw [rows][ld_pow] = re^2 + im^2
__global__ __launch_bounds__(256) void spk_power_kernel(const float* spec, int ld_spec, float* pw, int ld_pow, int64_t total, int nbins) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t r = i / nbins;
  const int k = (int)(i - r * nbins);
  const float re = spec[r * ld_spec + k], im = spec[r * ld_spec + nbins + k];
  pw[r * ld_pow + k] = re * re + im * im;
}

// mel [B][T][ld_mel] -> out [B][T][ldo] = log(max(mel, FLT_EPSILON)) (- its mean over the sequence's own frames when cmn);
// frames t >= len[b] are written as 0.  One workgroup per sequence: (bin, phase) threads sum rows t = phase (mod P) in
// order, the P partials are added in phase order.
__global__ __launch_bounds__(1024) void spk_log_cmn_kernel(const float* mel, int ld_mel, const int32_t* len, int T, int n_mels, int cmn,
                                                           float* out, int ldo) {
  __shared__ float part[1024];
  __shared__ float mean[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(len[b], 0), T);
  const float* mb = mel + (int64_t)b * T * ld_mel;
  float* ob = out + (int64_t)b * T * ldo;
  const int P = 1024 / n_mels;
  if (cmn) {
    const int c = tid % n_mels, ph = tid / n_mels;
    float s = 0.f;
    if (ph < P)
      for (int t = ph; t < n; t += P) s += logf(fmaxf(mb[(int64_t)t * ld_mel + c], FLT_EPSILON));
    part[tid] = s;
    __syncthreads();
    if (tid < n_mels) {
      float a = 0.f;
      for (int q = 0; q < P; ++q) a += part[q * n_mels + tid];
      mean[tid] = a / (float)max(n, 1);
    }
    __syncthreads();
  }
  for (int64_t i = tid; i < (int64_t)T * n_mels; i += 1024) {
    const int t = (int)(i / n_mels), c = (int)(i - (int64_t)t * n_mels);
    float v = 0.f;
    if (t < n) {
      v = logf(fmaxf(mb[(int64_t)t * ld_mel + c], FLT_EPSILON));
      if (cmn) v -= mean[c];
    }
    ob[(int64_t)t * ldo + c] = v;
  }
}

__device__ __forceinline__ float4 pre_relu(float4 a, const float* sc, const float* sh, int ci) {
  const float4 s = *(const float4*)(sc + ci), h = *(const float4*)(sh + ci);
  return make_float4(fmaxf(fmaf(a.x, s.x, h.x), 0.f), fmaxf(fmaf(a.y, s.y, h.y), 0.f), fmaxf(fmaf(a.z, s.z, h.z), 0.f),
                     fmaxf(fmaf(a.w, s.w, h.w), 0.f));
}

// Implicit-GEMM convolution, exact-f32 MFMA (v_mfma_f32_16x16x4_f32).  Output row m = t * F_out + f of sequence b, 32 output
// channels per wave (two 16-column accumulators sharing the A fragment), 16 rows per wave, four waves per workgroup.
// Lane l loads the A float4 of row (l & 15) at k = 16 i + 4 (l >> 4) and the matching W float4 of columns (l & 15) and 16 + (l & 15).
// K order: k = (i_f * kt + i_t) * cin + ci.  CIN1: a single input channel, K = kf * kt <= 16 taps in one 16-wide step.
template <bool CIN1>
__global__ __launch_bounds__(256) void spk_conv_kernel(const cv_spk_conv_params p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.z, n0 = blockIdx.y * 32;
  const int M = p.T_out * p.F_out;
  const int m0 = (blockIdx.x * 4 + wave) * 16;
  if (m0 >= M) return;
  const int in_len = p.in_len ? min(max(p.in_len[b], 0), p.T_in) : p.T_in;
  const int out_len = p.out_len ? min(max(p.out_len[b], 0), p.T_out) : p.T_out;
  const int ma = m0 + (lane & 15), kq = lane >> 4;
  const bool row_ok = ma < M;
  const int ta = row_ok ? ma / p.F_out : 0, fa = row_ok ? ma - ta * p.F_out : 0;
  const float* xb = p.x + (int64_t)b * p.x_bs;
  const float* w0 = p.w + (int64_t)(n0 + (lane & 15)) * p.ldw + 4 * kq;
  const float* w1 = w0 + (int64_t)16 * p.ldw;
  f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  if constexpr (CIN1) {
    float a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tap = 4 * kq + j;
      a[j] = 0.f;
      if (row_ok && tap < p.kf * p.kt) {
        const int i_f = tap / p.kt, i_t = tap - i_f * p.kt;
        const int fi = fa * p.sf + i_f - p.pf, ti = ta * p.st + i_t * p.dt - p.pt;
        if (fi >= 0 && fi < p.F_in && ti >= 0 && ti < in_len) {
          float v = xb[((int64_t)ti * p.F_in + fi) * p.ldx];
          if (p.pre_scale) v = fmaxf(fmaf(v, p.pre_scale[0], p.pre_shift[0]), 0.f);
          a[j] = v;
        }
      }
    }
    const float4 av = make_float4(a[0], a[1], a[2], a[3]);
    acc0 = mfma_block<CV_F32>(bitcast<uint4>(av), *(const uint4*)w0, acc0);
    acc1 = mfma_block<CV_F32>(bitcast<uint4>(av), *(const uint4*)w1, acc1);
  } else {
    for (int i_f = 0; i_f < p.kf; ++i_f) {
      for (int i_t = 0; i_t < p.kt; ++i_t) {
        const int fi = fa * p.sf + i_f - p.pf, ti = ta * p.st + i_t * p.dt - p.pt;
        const bool ok = row_ok && fi >= 0 && fi < p.F_in && ti >= 0 && ti < in_len;
        // out-of-range taps load row 0 (always valid memory) and are zeroed after the load: no branch in the K loop
        const float* xr = xb + ((int64_t)(ok ? ti : 0) * p.F_in + (ok ? fi : 0)) * p.ldx + 4 * kq;
        const int kb = (i_f * p.kt + i_t) * p.cin;
#pragma unroll 4
        for (int c0 = 0; c0 < p.cin; c0 += 16) {
          float4 a = *(const float4*)(xr + c0);
          if (p.pre_scale) a = pre_relu(a, p.pre_scale, p.pre_shift, c0 + 4 * kq);
          if (!ok) a = make_float4(0.f, 0.f, 0.f, 0.f);
          acc0 = mfma_block<CV_F32>(bitcast<uint4>(a), *(const uint4*)(w0 + kb + c0), acc0);
          acc1 = mfma_block<CV_F32>(bitcast<uint4>(a), *(const uint4*)(w1 + kb + c0), acc1);
        }
      }
    }
  }
  // epilogue: lane holds rows m0 + 4 (l >> 4) + r, columns n0 + (l & 15) and n0 + 16 + (l & 15)
  float* yb = p.y + (int64_t)b * p.y_bs;
  float ps[2] = {0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + 4 * kq + r;
    if (m >= M) continue;
    const int t = m / p.F_out;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int n = n0 + 16 * s + (lane & 15);
      float v = 0.f;
      if (t < out_len) {
        v = s ? acc1[r] : acc0[r];
        if (p.bias) v += p.bias[n];
        if (p.res) v += p.res[(int64_t)b * p.res_bs + (int64_t)m * p.ldres + n];
        if (p.relu) v = fmaxf(v, 0.f);
        if (p.gate) v *= p.gate[(int64_t)b * p.gate_bs + (int64_t)(t / p.gate_seg) * p.N + n];
      }
      yb[(int64_t)m * p.ldy + n] = v;
      ps[s] += v;
    }
  }
  if (p.psum) {   // F_out == 1: the lane's four rows are one aligned group of 4 time steps
    const int g = (m0 >> 2) + kq;
    if (4 * g < p.T_out) {
      float* pb = p.psum + (int64_t)b * p.psum_bs + (int64_t)g * p.N + n0 + (lane & 15);
      pb[0] = ps[0];
      pb[16] = ps[1];
    }
  }
}

// CAM context gate (CAMPPlus.py:95-112): context = mean over the sequence + mean over its segment (avg_pool1d ceil_mode: the
// last segment averages its valid frames only), m = sigmoid(W2 relu(W1 context + b1) + b2).  From the 4-row group sums psum
// [B][groups][128] of the bottleneck activation.  One workgroup per (segment, sequence); every sum is split over a fixed number
// of thread slices whose partials are added in slice order (deterministic, independent of the padded length).
__global__ __launch_bounds__(512) void spk_cam_gate_kernel(const float* psum, int64_t psum_bs, const int32_t* len, int T, int seg_len,
                                                           const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                                                           int64_t gate_bs) {
  __shared__ float part[2][4][128];
  __shared__ float ctx[128];
  __shared__ float hp[8][64];
  __shared__ float hid[64];
  __shared__ float op[8][32];
  const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(len[b], 0), T);
  float* g = gate + (int64_t)b * gate_bs + (int64_t)s * 32;
  if (s * seg_len >= n) {   // a segment past the sequence: never read (its rows are masked), written for determinism
    if (tid < 32) g[tid] = 0.f;
    return;
  }
  const float* ps = psum + (int64_t)b * psum_bs;
  const int groups = (n + 3) >> 2, g0 = s * (seg_len >> 2), g1 = min(groups, (s + 1) * (seg_len >> 2));
  {
    const int c = tid & 127, ph = tid >> 7;   // 4 slices of groups per channel
    float tot = 0.f, seg = 0.f;
#pragma unroll 8
    for (int i = ph; i < groups; i += 4) tot += ps[(int64_t)i * 128 + c];
#pragma unroll 8
    for (int i = g0 + ph; i < g1; i += 4) seg += ps[(int64_t)i * 128 + c];
    part[0][ph][c] = tot;
    part[1][ph][c] = seg;
  }
  __syncthreads();
  if (tid < 128) {
    const float tot = ((part[0][0][tid] + part[0][1][tid]) + part[0][2][tid]) + part[0][3][tid];
    const float seg = ((part[1][0][tid] + part[1][1][tid]) + part[1][2][tid]) + part[1][3][tid];
    ctx[tid] = tot / (float)n + seg / (float)min(seg_len, n - s * seg_len);
  }
  __syncthreads();
  {
    const int j = tid & 63, sl = tid >> 6;     // 64 hidden x 8 slices of 16 context channels
    const float* wr = w1 + j * 128 + sl * 16;
    float h = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) h = fmaf(wr[k], ctx[sl * 16 + k], h);
    hp[sl][j] = h;
  }
  __syncthreads();
  if (tid < 64) {
    float h = b1[tid];
    for (int q = 0; q < 8; ++q) h += hp[q][tid];
    hid[tid] = fmaxf(h, 0.f);
  }
  __syncthreads();
  if (tid < 256) {
    const int o = tid & 31, sl = tid >> 5;     // 32 outputs x 8 slices of 8 hidden
    const float* wr = w2 + o * 64 + sl * 8;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v = fmaf(wr[k], hid[sl * 8 + k], v);
    op[sl][o] = v;
  }
  __syncthreads();
  if (tid < 32) {
    float v = b2[tid];
    for (int q = 0; q < 8; ++q) v += op[q][tid];
    g[tid] = 1.f / (1.f + expf(-v));
  }
}

// out_nonlinear (BN -> ReLU, CAMPPlus.py:436-437) fused into statistics pooling (:35-46): out[b] = [mean | unbiased std] over
// the sequence's own rows.  Workgroup = 64 channels x 4 row phases; phase partials are added in phase order.
__global__ __launch_bounds__(256) void spk_stats_kernel(const float* x, int64_t x_bs, int ldx, const int32_t* len, int T, int C,
                                                        const float* sc, const float* sh, float* out, int64_t out_bs) {
  __shared__ float part[4][64];
  const int b = blockIdx.y, cl = threadIdx.x & 63, ph = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  const int n = min(max(len[b], 0), T);
  const float* xb = x + (int64_t)b * x_bs + c;
  const bool pre = sc != nullptr;   // without the prologue the rows are pooled as they are: no ReLU either
  const float s_ = pre ? sc[c] : 1.f, h_ = pre ? sh[c] : 0.f;
  float s = 0.f;
  for (int t = ph; t < n; t += 4) {
    const float v = xb[(int64_t)t * ldx];
    s += pre ? fmaxf(fmaf(v, s_, h_), 0.f) : v;
  }
  part[ph][cl] = s;
  __syncthreads();
  const float mean = (part[0][cl] + part[1][cl] + part[2][cl] + part[3][cl]) / (float)n;
  __syncthreads();
  float q = 0.f;
  for (int t = ph; t < n; t += 4) {
    const float v = xb[(int64_t)t * ldx];
    const float d = (pre ? fmaxf(fmaf(v, s_, h_), 0.f) : v) - mean;
    q = fmaf(d, d, q);
  }
  part[ph][cl] = q;
  __syncthreads();
  if (ph == 0) {
    const float var = (part[0][cl] + part[1][cl] + part[2][cl] + part[3][cl]) / (float)(n - 1);
    out[(int64_t)b * out_bs + c] = mean;
    out[(int64_t)b * out_bs + C + c] = sqrtf(var);
  }
}

}  // namespace

extern "C" int cv_sizeof_spk_conv_params(void) { return (int)sizeof(cv_spk_conv_params); }

extern "C" int cv_spk_power(const float* spec, int32_t ld_spec, float* pw, int32_t ld_pow, int32_t rows, int32_t nbins, void* stream) {
  if (!spec || !pw || rows <= 0 || nbins <= 0 || ld_spec < 2 * nbins || ld_pow < nbins) return CV_ERR_ARG;
  const int64_t total = (int64_t)rows * nbins;
  hipLaunchKernelGGL(spk_power_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, spec, ld_spec, pw, ld_pow,
                     total, nbins);
  CV_CHECK_LAUNCH();
  return CV_OK;
}

extern "C" int cv_spk_log_cmn(const float* mel, int32_t ld_mel, const int32_t* len, int32_t B, int32_t T, int32_t n_mels, int32_t cmn,
                              float* out, int32_t ldo, void* stream) {
  if (!mel || !len || !out || B <= 0 || T <= 0 || n_mels <= 0 || n_mels > 256 || ld_mel < n_mels || ldo < n_mels || B > 65535)
    return CV_ERR_ARG;
  hipLaunchKernelGGL(spk_log_cmn_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, mel, ld_mel, len, T, n_mels, cmn, out, ldo);
  CV_CHECK_LAUNCH();
  return CV_OK;
}

extern "C" int cv_spk_conv(const cv_spk_conv_params* pp, void* stream) {
  if (!pp) return CV_ERR_ARG;
  const cv_spk_conv_params& p = *pp;
  if (!p.x || !p.w || !p.y || p.B <= 0 || p.B > 65535 || p.T_in <= 0 || p.F_in <= 0 || p.cin <= 0 || p.T_out <= 0 || p.F_out <= 0)
    return CV_ERR_ARG;
  if (p.kf <= 0 || p.kt <= 0 || p.sf <= 0 || p.st <= 0 || p.dt <= 0 || p.pf < 0 || p.pt < 0) return CV_ERR_ARG;
  if (p.N <= 0 || (p.N & 31) || p.ldy < p.N || p.ldx < p.cin || (p.ldw & 15) || p.ldw < p.kf * p.kt * p.cin) return CV_ERR_ARG;
  if ((int64_t)p.T_out * p.F_out > 0x7FFFFFFF - 64) return CV_ERR_ARG;
  const bool cin1 = p.cin == 1;
  if (cin1 ? p.kf * p.kt > 16 : ((p.cin & 15) || (p.ldx & 3) || (p.x_bs & 3) || ((uintptr_t)p.x & 15))) return CV_ERR_ARG;
  if ((uintptr_t)p.w & 15) return CV_ERR_ARG;
  if ((p.pre_scale == nullptr) != (p.pre_shift == nullptr)) return CV_ERR_ARG;
  if (!cin1 && p.pre_scale && (((uintptr_t)p.pre_scale & 15) || ((uintptr_t)p.pre_shift & 15))) return CV_ERR_ARG;
  if (p.res && p.ldres < p.N) return CV_ERR_ARG;
  if (p.gate && p.gate_seg <= 0) return CV_ERR_ARG;
  if (p.psum && (p.F_out != 1 || p.psum_bs < (int64_t)((p.T_out + 3) / 4) * p.N)) return CV_ERR_ARG;
  const int M = p.T_out * p.F_out;
  const dim3 grid((M + 63) / 64, p.N / 32, p.B);
  if (cin1) hipLaunchKernelGGL(spk_conv_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(spk_conv_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
  CV_CHECK_LAUNCH();
  return CV_OK;
}

extern "C" int cv_spk_cam_gate(const float* psum, int64_t psum_bs, const int32_t* len, int32_t B, int32_t T, int32_t seg_len,
                               const float* w1, const float* b1, const float* w2, const float* b2, float* gate, int64_t gate_bs,
                               void* stream) {
  if (!psum || !len || !w1 || !b1 || !w2 || !b2 || !gate || B <= 0 || B > 65535 || T <= 0 || seg_len <= 0 || (seg_len & 3)) return CV_ERR_ARG;
  const int nseg = (T + seg_len - 1) / seg_len;
  if (psum_bs < (int64_t)((T + 3) / 4) * 128 || gate_bs < (int64_t)nseg * 32) return CV_ERR_ARG;
  hipLaunchKernelGGL(spk_cam_gate_kernel, dim3(nseg, B), dim3(512), 0, (hipStream_t)stream, psum, psum_bs, len, T, seg_len, w1, b1, w2, b2,
                     gate, gate_bs);
  CV_CHECK_LAUNCH();
  return CV_OK;
}

extern "C" int cv_spk_stats_pool(const float* x, int64_t x_bs, int32_t ldx, const int32_t* len, int32_t B, int32_t T, int32_t C,
                                 const float* pre_scale, const float* pre_shift, float* out, int64_t out_bs, void* stream) {
  if (!x || !len || !out || B <= 0 || B > 65535 || T <= 0 || C <= 0 || (C & 63) || ldx < C || out_bs < 2 * (int64_t)C) return CV_ERR_ARG;
  if ((pre_scale == nullptr) != (pre_shift == nullptr)) return CV_ERR_ARG;
  hipLaunchKernelGGL(spk_stats_kernel, dim3(C / 64, B), dim3(256), 0, (hipStream_t)stream, x, x_bs, ldx, len, T, C, pre_scale, pre_shift,
                     out, out_bs);
  CV_CHECK_LAUNCH();
  return CV_OK;
}
