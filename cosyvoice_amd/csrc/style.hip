// Speaker encoder v2 (include/cosyvoice_amd_style.h): the WaveNet layer of the posterior encoder (cosyvoice/speaker/modules.py:197-218),
// Conv1dGLU (:498-515), the two attentions of the style branch (:577-630, :689-710), the posterior sample
// (posterior_encoder.py:35-36) and the masked temporal mean (style_encoder.py:73-81).
//
// Row-block structure of cv_wn_layer / cv_glu_conv: a workgroup of 8 waves owns 32 rows of one sequence.  The rows and their
// 2-row halo are staged in LDS once (rows outside [0, len) as zeros: the conv padding and the x * mask of the previous layer at
// once); wave w computes gate columns [w C / 8, (w + 1) C / 8) of both conv halves, 16 columns x 32 rows x 2 halves = four
// accumulators at a time, streaming the weights L2 -> VGPR; the gate product goes to a second LDS image, which is the A operand of
// the 1x1 GEMM.  Exact-f32 MFMA throughout: an output element is one k-ordered fma chain whatever tile it lands in.
#include <float.h>
#include "cv_device.h"
#include "../../include/cosyvoice_amd_style.h"

namespace {

constexpr int ROWS = 32, HALO = 2, TAPS = 5, NW = 8, NTHR = NW * 64;
constexpr int WN_C = 512, GLU_C = 256;
constexpr int ATT_MAX_T = 2400;

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// rows t0 - 2 .. t0 + 33 of one sequence -> xs [36][C + 4]; rows outside [0, len) are zeros and are not read
template <int C>
__device__ __forceinline__ void stage_rows(float* xs, const float* xb, int ldx, int t0, int len, int tid) {
  constexpr int P = C + 4, V = C / 4;
  for (int i = tid; i < (ROWS + 2 * HALO) * V; i += NTHR) {
    const int r = i / V, c = (i - r * V) * 4;
    const int t = t0 - HALO + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t >= 0 && t < len) v = *(const float4*)(xb + (int64_t)t * ldx + c);
    *(float4*)(xs + r * P + c) = v;
  }
}

// acc[mi][h] += rows 16 mi .. 16 mi + 15 of the staged tile (*) columns n (h = 0) and n + C (h = 1) of w [2C][TAPS * C]
template <int C>
__device__ __forceinline__ void conv_pair(const float* xs, const float* w, int n, int lane, f32x4_t (&acc)[2][2]) {
  constexpr int P = C + 4, K = TAPS * C;
  const int lq = lane & 15, kq = lane >> 4;
  const float* wa = w + (int64_t)n * K + 4 * kq;
  const float* wb = wa + (int64_t)C * K;
  for (int tap = 0; tap < TAPS; ++tap) {
    const float* a0 = xs + (lq + tap) * P + 4 * kq;   // output row r reads staged row r + tap (= t - 2 + tap)
    const float* a1 = a0 + 16 * P;
    const float* wat = wa + tap * C;
    const float* wbt = wb + tap * C;
#pragma unroll 4
    for (int c0 = 0; c0 < C; c0 += 16) {
      const uint4 A0 = *(const uint4*)(a0 + c0), A1 = *(const uint4*)(a1 + c0);
      const uint4 Wa = *(const uint4*)(wat + c0), Wb = *(const uint4*)(wbt + c0);
      acc[0][0] = mfma_block<CV_F32>(A0, Wa, acc[0][0]);
      acc[1][0] = mfma_block<CV_F32>(A1, Wa, acc[1][0]);
      acc[0][1] = mfma_block<CV_F32>(A0, Wb, acc[0][1]);
      acc[1][1] = mfma_block<CV_F32>(A1, Wb, acc[1][1]);
    }
  }
}

__device__ __forceinline__ void zero_rows(float* dst, int ld, int rows, int C, int tid) {
  const int V = C / 4;
  for (int i = tid; i < rows * V; i += NTHR) {
    const int r = i / V, c = (i - r * V) * 4;
    *(float4*)(dst + (int64_t)r * ld + c) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__global__ __launch_bounds__(NTHR) void wn_layer_kernel(const cv_wn_layer_params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int C = WN_C, P = C + 4;
  float* xs = (float*)smem;                    // [36][P] input rows with halo
  float* gs = xs + (ROWS + 2 * HALO) * P;      // [32][P] gate product
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 15, kq = lane >> 4;
  const int b = blockIdx.y, t0 = blockIdx.x * ROWS;
  const int len = min(max(p.len[b], 0), p.T);
  const int rows = min(ROWS, p.T - t0);
  const bool res = p.n_rs == 2 * C;
  float* xo = res ? p.x_out + (int64_t)b * p.xo_bs + (int64_t)t0 * p.ldxo : nullptr;
  float* sk = p.skip + (int64_t)b * p.skip_bs + (int64_t)t0 * p.ldskip;
  if (t0 >= len) {   // a tile past the sequence: zeros, nothing read
    if (res) zero_rows(xo, p.ldxo, rows, C, tid);
    zero_rows(sk, p.ldskip, rows, C, tid);
    return;
  }
  stage_rows<C>(xs, p.x + (int64_t)b * p.x_bs, p.ldx, t0, len, tid);
  __syncthreads();
  for (int ns = 0; ns < C / NW / 16; ++ns) {
    const int n = wave * (C / NW) + ns * 16 + lq;
    f32x4_t acc[2][2] = {};
    conv_pair<C>(xs, p.w_in, n, lane, acc);
    const float ba = p.b_in[n], bb = p.b_in[n + C];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        gs[(mi * 16 + 4 * kq + r) * P + n] = tanhf(acc[mi][0][r] + ba) * sigmoidf_(acc[mi][1][r] + bb);
  }
  __syncthreads();
  const int per_wave = p.n_rs / NW;   // 128 or 64 columns of the 1x1
  for (int n0 = wave * per_wave; n0 < (wave + 1) * per_wave; n0 += 32) {
    f32x4_t acc[2][2] = {};
    const float* w0 = p.w_rs + (int64_t)(n0 + lq) * C + 4 * kq;
    const float* w1 = w0 + 16 * C;
    const float* g0 = gs + lq * P + 4 * kq;
    const float* g1 = g0 + 16 * P;
#pragma unroll 4
    for (int c0 = 0; c0 < C; c0 += 16) {
      const uint4 A0 = *(const uint4*)(g0 + c0), A1 = *(const uint4*)(g1 + c0);
      const uint4 W0 = *(const uint4*)(w0 + c0), W1 = *(const uint4*)(w1 + c0);
      acc[0][0] = mfma_block<CV_F32>(A0, W0, acc[0][0]);
      acc[1][0] = mfma_block<CV_F32>(A1, W0, acc[1][0]);
      acc[0][1] = mfma_block<CV_F32>(A0, W1, acc[0][1]);
      acc[1][1] = mfma_block<CV_F32>(A1, W1, acc[1][1]);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int n = n0 + 16 * s + lq;
      const float bias = p.b_rs[n];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = mi * 16 + 4 * kq + r;
          if (row >= rows) continue;
          const bool live = t0 + row < len;
          const float v = acc[mi][s][r] + bias;
          if (res && n < C) {
            xo[(int64_t)row * p.ldxo + n] = live ? xs[(row + HALO) * P + n] + v : 0.f;
          } else {
            float* d = sk + (int64_t)row * p.ldskip + (res ? n - C : n);
            *d = live ? (p.skip_init ? v : *d + v) : 0.f;
          }
        }
    }
  }
}

__global__ __launch_bounds__(256) void wn_gate_kernel(const float* a, int lda, float* g, int ldg, int C, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t row = i / C;
  const int c = (int)(i - row * C);
  const float* ar = a + row * lda;
  g[row * ldg + c] = tanhf(ar[c]) * sigmoidf_(ar[C + c]);
}

__global__ __launch_bounds__(NTHR) void glu_conv_kernel(const cv_glu_conv_params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int C = GLU_C, P = C + 4;
  float* xs = (float*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 15, kq = lane >> 4;
  const int b = blockIdx.y, t0 = blockIdx.x * ROWS;
  const int len = min(max(p.len[b], 0), p.T);
  const int rows = min(ROWS, p.T - t0);
  float* y = p.y + (int64_t)b * p.y_bs + (int64_t)t0 * p.ldy;
  if (t0 >= len) {
    zero_rows(y, p.ldy, rows, C, tid);
    return;
  }
  stage_rows<C>(xs, p.x + (int64_t)b * p.x_bs, p.ldx, t0, len, tid);
  __syncthreads();
  for (int ns = 0; ns < C / NW / 16; ++ns) {
    const int n = wave * (C / NW) + ns * 16 + lq;
    f32x4_t acc[2][2] = {};
    conv_pair<C>(xs, p.w, n, lane, acc);
    const float ba = p.bias[n], bb = p.bias[n + C];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mi * 16 + 4 * kq + r;
        if (row >= rows) continue;
        const float g = (acc[mi][0][r] + ba) * sigmoidf_(acc[mi][1][r] + bb);
        y[(int64_t)row * p.ldy + n] = t0 + row < len ? xs[(row + HALO) * P + n] + g : 0.f;
      }
  }
}

// One query row against n_tok fixed keys / values of one head.  256 threads: scores by token (thread t, t + 256, ...: one fma chain
// over d each), max and sum over per-thread partials combined in thread order, then (d, 4 token phases) for the value sum.
__global__ __launch_bounds__(256) void gst_attention_kernel(const float* q, int ldq, const float* k, const float* v, float* out, int ldo,
                                                            int n_tok, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sc = (float*)smem;          // [n_tok]
  __shared__ float qs[64];
  __shared__ float red[256];
  __shared__ float part[4][64];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* kh = k + (int64_t)h * n_tok * 64;
  const float* vh = v + (int64_t)h * n_tok * 64;
  if (tid < 64) qs[tid] = q[(int64_t)b * ldq + h * 64 + tid];
  __syncthreads();
  float mx = -FLT_MAX;
  for (int t = tid; t < n_tok; t += 256) {
    const float4* kr = (const float4*)(kh + (int64_t)t * 64);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float4 kk = kr[i];
      s = fmaf(qs[4 * i], kk.x, s);
      s = fmaf(qs[4 * i + 1], kk.y, s);
      s = fmaf(qs[4 * i + 2], kk.z, s);
      s = fmaf(qs[4 * i + 3], kk.w, s);
    }
    s *= scale;
    sc[t] = s;
    mx = fmaxf(mx, s);
  }
  red[tid] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]);
    __syncthreads();
  }
  mx = red[0];
  __syncthreads();
  float sum = 0.f;
  for (int t = tid; t < n_tok; t += 256) {
    const float e = expf(sc[t] - mx);
    sc[t] = e;
    sum += e;
  }
  red[tid] = sum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  sum = red[0];
  const int d = tid & 63, ph = tid >> 6;
  float a = 0.f;
  for (int t = ph; t < n_tok; t += 4) a = fmaf(sc[t], vh[(int64_t)t * 64 + d], a);
  part[ph][d] = a;
  __syncthreads();
  if (ph == 0) out[(int64_t)b * ldo + h * 64 + d] = (((part[0][d] + part[1][d]) + part[2][d]) + part[3][d]) / sum;
}

// 16 query rows of one (head, sequence) per workgroup of 4 waves.  S = Q K^T: wave w takes key tiles w, w + 4, ... (Q fragments in
// registers); softmax: 16 threads per row, partials combined by a fixed xor tree; O = P V: wave w takes d columns [16 w, 16 w + 16),
// keys in order.  Keys at or past len are never read (P = 0 there and V is replaced by 0).
__global__ __launch_bounds__(256) void style_attention_kernel(const float* q, const float* k, const float* v, int64_t qkv_bs, int ld, float* out,
                                                              int64_t o_bs, int ldo, const int32_t* lens, int T, float scale, int pitch) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sc = (float*)smem;          // [16][pitch]
  __shared__ float inv[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, kq = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, t0 = blockIdx.x * 16;
  const int len = min(max(lens[b], 0), T);
  const int rows = min(16, T - t0);
  float* ob = out + (int64_t)b * o_bs + (int64_t)t0 * ldo + h * 64;
  if (t0 >= len) {
    for (int i = tid; i < rows * 64; i += 256) ob[(int64_t)(i >> 6) * ldo + (i & 63)] = 0.f;
    return;
  }
  const float* qb = q + (int64_t)b * qkv_bs + h * 64;
  const float* kb = k + (int64_t)b * qkv_bs + h * 64;
  const float* vb = v + (int64_t)b * qkv_bs + h * 64;
  const int nkt = (len + 15) >> 4;   // key tiles that hold a live key
  uint4 qf[4];
  {
    const int t = t0 + lq;
    const bool ok = t < len;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok) f = *(const float4*)(qb + (int64_t)t * ld + 16 * i + 4 * kq);
      qf[i] = bitcast<uint4>(f);
    }
  }
  for (int kt = wave; kt < nkt; kt += 4) {
    const int key = kt * 16 + lq;
    const bool ok = key < len;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float4 f = *(const float4*)(kb + (int64_t)min(key, len - 1) * ld + 16 * i + 4 * kq);   // unconditional load, clamped row
      if (!ok) f = make_float4(0.f, 0.f, 0.f, 0.f);
      acc = mfma_block<CV_F32>(qf[i], bitcast<uint4>(f), acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[(4 * kq + r) * pitch + key] = ok ? acc[r] * scale : -FLT_MAX;
  }
  __syncthreads();
  {
    const int row = tid >> 4, sub = tid & 15;
    float* sr = sc + row * pitch;
    float mx = -FLT_MAX;
    for (int j = sub; j < len; j += 16) mx = fmaxf(mx, sr[j]);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 16));
    float sum = 0.f;
    for (int j = sub; j < nkt * 16; j += 16) {
      const float e = j < len ? expf(sr[j] - mx) : 0.f;
      sr[j] = e;
      if (j < len) sum += e;
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 16);
    if (sub == 0) inv[row] = 1.0f / sum;
  }
  __syncthreads();
  {
    const int d = wave * 16 + lq;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    const float* pr = sc + lq * pitch + 4 * kq;
    for (int kt = 0; kt < nkt; ++kt) {
      const uint4 P = *(const uint4*)(pr + kt * 16);
      const int key = kt * 16 + 4 * kq;
      float4 vv;   // unconditional loads of clamped rows; a key at or past len contributes an exact 0 (P is 0 there as well)
      vv.x = vb[(int64_t)min(key, len - 1) * ld + d];
      vv.y = vb[(int64_t)min(key + 1, len - 1) * ld + d];
      vv.z = vb[(int64_t)min(key + 2, len - 1) * ld + d];
      vv.w = vb[(int64_t)min(key + 3, len - 1) * ld + d];
      if (key >= len) vv.x = 0.f;
      if (key + 1 >= len) vv.y = 0.f;
      if (key + 2 >= len) vv.z = 0.f;
      if (key + 3 >= len) vv.w = 0.f;
      acc = mfma_block<CV_F32>(P, bitcast<uint4>(vv), acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * kq + r;
      if (row >= rows) continue;
      ob[(int64_t)row * ldo + d] = t0 + row < len ? acc[r] * inv[row] : 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void posterior_sample_kernel(const float* stats, int ld_stats, const float* noise, float* z, int ldz,
                                                               const int32_t* lens, int T, int C, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t row = i / C;
  const int c = (int)(i - row * C);
  const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
  float val = 0.f;
  if (t < min(max(lens[b], 0), T)) {
    const float* s = stats + row * ld_stats;
    val = s[c] + noise[row * C + c] * expf(s[C + c]);
  }
  z[row * ldz + c] = val;
}

__global__ __launch_bounds__(256) void masked_mean_kernel(const float* x, int64_t x_bs, int ldx, const int32_t* lens, int T, float* out,
                                                          int ldo) {
  __shared__ float part[4][64];
  const int b = blockIdx.y, cl = threadIdx.x & 63, ph = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  const int n = min(max(lens[b], 0), T);
  const float* xb = x + (int64_t)b * x_bs + c;
  float s = 0.f;
  for (int t = ph; t < n; t += 4) s += xb[(int64_t)t * ldx];
  part[ph][cl] = s;
  __syncthreads();
  if (ph == 0) out[(int64_t)b * ldo + c] = n > 0 ? (((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl]) / (float)n : 0.f;
}

constexpr size_t WN_LDS = (size_t)(2 * ROWS + 2 * HALO) * (WN_C + 4) * sizeof(float);
constexpr size_t GLU_LDS = (size_t)(ROWS + 2 * HALO) * (GLU_C + 4) * sizeof(float);

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int cv_sizeof_wn_layer_params(void) { return (int)sizeof(cv_wn_layer_params); }
extern "C" int cv_sizeof_glu_conv_params(void) { return (int)sizeof(cv_glu_conv_params); }

extern "C" int cv_wn_layer(const cv_wn_layer_params* pp, void* stream) {
  if (!pp) return CV_ERR_ARG;
  const cv_wn_layer_params& p = *pp;
  if (p.B <= 0 || p.B > 65535 || p.T <= 0 || p.C <= 0 || p.taps <= 0) return CV_ERR_ARG;
  if (!p.len || !p.x || !p.w_in || !p.b_in || !p.w_rs || !p.b_rs || !p.skip) return CV_ERR_ARG;
  if (p.C != WN_C || p.taps != TAPS) return CV_ERR_UNSUPPORTED;
  if (p.n_rs != p.C && p.n_rs != 2 * p.C) return CV_ERR_ARG;
  const bool res = p.n_rs == 2 * p.C;
  if (res && (!p.x_out || p.x_out == p.x || p.ldxo < p.C || (p.ldxo & 3) || (p.xo_bs & 3) || !aligned16(p.x_out))) return CV_ERR_ARG;
  if (p.ldx < p.C || (p.ldx & 3) || (p.x_bs & 3) || !aligned16(p.x) || !aligned16(p.w_in) || !aligned16(p.w_rs)) return CV_ERR_ARG;
  if (p.ldskip < p.C || (p.ldskip & 3) || (p.skip_bs & 3) || !aligned16(p.skip)) return CV_ERR_ARG;
  static PerDeviceOnce once;   // > 64 KiB of dynamic LDS needs the opt-in
  once.run([] { hipFuncSetAttribute((const void*)wn_layer_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WN_LDS); });
  hipLaunchKernelGGL(wn_layer_kernel, dim3((p.T + ROWS - 1) / ROWS, p.B), dim3(NTHR), WN_LDS, (hipStream_t)stream, p);
  CV_CHECK_LAUNCH();
  return CV_OK;
}

extern "C" int cv_wn_gate(const float* a, int32_t lda, float* g, int32_t ldg, int32_t rows, int32_t C, void* stream) {
  if (!a || !g || rows <= 0 || C <= 0 || lda < 2 * C || ldg < C) return CV_ERR_ARG;
  const int64_t total = (int64_t)rows * C;
  if ((total + 255) / 256 > 0x7FFFFFFF) return CV_ERR_ARG;
  hipLaunchKernelGGL(wn_gate_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, lda, g, ldg, C, total);
  CV_CHECK_LAUNCH();
  return CV_OK;
}

extern "C" int cv_glu_conv(const cv_glu_conv_params* pp, void* stream) {
  if (!pp) return CV_ERR_ARG;
  const cv_glu_conv_params& p = *pp;
  if (p.B <= 0 || p.B > 65535 || p.T <= 0 || p.C <= 0 || p.taps <= 0) return CV_ERR_ARG;
  if (!p.len || !p.x || !p.w || !p.bias || !p.y || p.y == p.x) return CV_ERR_ARG;
  if (p.C != GLU_C || p.taps != TAPS) return CV_ERR_UNSUPPORTED;
  if (p.ldx < p.C || (p.ldx & 3) || (p.x_bs & 3) || !aligned16(p.x) || !aligned16(p.w)) return CV_ERR_ARG;
  if (p.ldy < p.C || (p.ldy & 3) || (p.y_bs & 3) || !aligned16(p.y)) return CV_ERR_ARG;
  hipLaunchKernelGGL(glu_conv_kernel, dim3((p.T + ROWS - 1) / ROWS, p.B), dim3(NTHR), GLU_LDS, (hipStream_t)stream, p);
  CV_CHECK_LAUNCH();
  return CV_OK;
}

extern "C" int cv_gst_attention(const float* q, int32_t ldq, const float* k, const float* v, float* out, int32_t ldo, int32_t B, int32_t H,
                                int32_t n_tok, float scale, void* stream) {
  if (!q || !k || !v || !out || B <= 0 || B > 65535 || H <= 0 || n_tok <= 0 || ldq < H * 64 || ldo < H * 64) return CV_ERR_ARG;
  if (!aligned16(k)) return CV_ERR_ARG;
  if (n_tok > 8192) return CV_ERR_UNSUPPORTED;   // the score row lives in LDS
  hipLaunchKernelGGL(gst_attention_kernel, dim3(H, B), dim3(256), (size_t)n_tok * sizeof(float), (hipStream_t)stream, q, ldq, k, v, out, ldo,
                     n_tok, scale);
  CV_CHECK_LAUNCH();
  return CV_OK;
}

extern "C" int cv_style_attention(const float* q, const float* k, const float* v, int64_t qkv_bs, int32_t ld, float* out, int64_t o_bs,
                                  int32_t ldo, const int32_t* len, int32_t B, int32_t T, int32_t H, float scale, void* stream) {
  if (!q || !k || !v || !out || !len || B <= 0 || B > 65535 || T <= 0 || H <= 0 || H > 65535 || ld < H * 64 || ldo < H * 64) return CV_ERR_ARG;
  if ((ld & 3) || (qkv_bs & 3) || !aligned16(q) || !aligned16(k)) return CV_ERR_ARG;
  if (T > ATT_MAX_T) return CV_ERR_UNSUPPORTED;
  const int pitch = ((T + 15) & ~15) + 4;
  const size_t lds = (size_t)16 * pitch * sizeof(float);
  static PerDeviceOnce once;
  once.run([] {
    hipFuncSetAttribute((const void*)style_attention_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)((size_t)16 * (ATT_MAX_T + 4) * sizeof(float)));
  });
  hipLaunchKernelGGL(style_attention_kernel, dim3((T + 15) / 16, H, B), dim3(256), lds, (hipStream_t)stream, q, k, v, qkv_bs, ld, out, o_bs,
                     ldo, len, T, scale, pitch);
  CV_CHECK_LAUNCH();
  return CV_OK;
}

extern "C" int cv_posterior_sample(const float* stats, int32_t ld_stats, const float* noise, float* z, int32_t ldz, const int32_t* len,
                                   int32_t B, int32_t T, int32_t C, void* stream) {
  if (!stats || !noise || !z || !len || B <= 0 || T <= 0 || C <= 0 || ld_stats < 2 * C || ldz < C) return CV_ERR_ARG;
  const int64_t total = (int64_t)B * T * C;
  if ((total + 255) / 256 > 0x7FFFFFFF) return CV_ERR_ARG;
  hipLaunchKernelGGL(posterior_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, stats, ld_stats, noise,
                     z, ldz, len, T, C, total);
  CV_CHECK_LAUNCH();
  return CV_OK;
}

extern "C" int cv_masked_mean(const float* x, int64_t x_bs, int32_t ldx, const int32_t* len, int32_t B, int32_t T, int32_t C, float* out,
                              int32_t ldo, void* stream) {
  if (!x || !len || !out || B <= 0 || B > 65535 || T <= 0 || C <= 0 || (C & 63) || ldx < C || ldo < C) return CV_ERR_ARG;
  hipLaunchKernelGGL(masked_mean_kernel, dim3(C / 64, B), dim3(256), 0, (hipStream_t)stream, x, x_bs, ldx, len, T, out, ldo);
  CV_CHECK_LAUNCH();
  return CV_OK;
}
