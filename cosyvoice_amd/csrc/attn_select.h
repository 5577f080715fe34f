// cv_attention, steps one and two of three: check the parameter block, then pick the kernel form, waves, grid and LDS size.  Plain C++17
// over the public header only (see skinny_select.h); step three is the launch in attention.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/cosyvoice_amd.h"

constexpr int ATTN_STAGE_BYTES = 16384;   // one K tile + one V^T tile of 64 keys (attention.hip: KT_BYTES + VT_BYTES)

struct AttnSel {
  int form;    // 16: attn_kernel, 32: attn32_kernel, 64: attn64_kernel
  int waves;   // waves per workgroup (the 64 form: 4), 64 queries per wave in form 64, 32 otherwise
  unsigned grid_x, grid_y, grid_z, block;
  size_t lds;
};

// Defaults (q_hs / k_hs 0 -> 64, written back into p) and checks, then the pick.  Returns CV_OK and fills *out, or cv_attention's code.
inline int attn_select(cv_attn_params& p, AttnSel* out) {
  if (p.q_hs == 0) p.q_hs = 64;
  if (p.k_hs == 0) p.k_hs = 64;
  if ((p.q_hs & 7) || (p.k_hs & 7)) return CV_ERR_ARG;
  if (p.dtype != CV_BF16 && p.dtype != CV_F16) return CV_ERR_UNSUPPORTED;
  if (p.B <= 0 || p.H <= 0 || p.Hkv <= 0 || (p.H % p.Hkv) || p.Tq <= 0 || p.Tk <= 0 || p.q_off < 0) return CV_ERR_ARG;
  if (!p.q || !p.k || !p.vt || !p.out) return CV_ERR_ARG;
  if ((p.ldq & 7) || (p.ldk & 7) || (p.vt_ld & 7) || (p.ldo & 3) || (p.q_bs & 7) || (p.k_bs & 7) || (p.o_bs & 3)) return CV_ERR_ARG;
  if (p.vt_ld < p.Tk) return CV_ERR_ARG;
  if ((int64_t)p.Tk * p.ldk * 2 >= (int64_t)1 << 31 || (int64_t)64 * p.vt_ld * 2 >= (int64_t)1 << 31) return CV_ERR_UNSUPPORTED;   // 32-bit buffer offsets per (batch, head)
  if (((uintptr_t)p.q & 15) || ((uintptr_t)p.k & 15) || ((uintptr_t)p.vt & 15) || ((uintptr_t)p.out & 7)) return CV_ERR_ARG;
  // p.mfma selects among the three forms (all tested against torch, tests/test_attention_gpu.py):
  //   0 / 16 the 16x16x32 form (the library's choice);
  //   32 the same tiling on 32x32x16 MFMAs (half the MFMA issue slots, one cross-lane step per row max): 58.2 vs 57.0 us;
  //   64 64 queries per wave, K / V^T by LDS-DMA into a 3-stage ring, the softmax of one query block issued between the MFMAs of the
  //      other (no bias operand): 57.0 - 58.2 us.
  // At the estimator's batch-8 shape (16 x 8 heads x T = 1000) all three take 57 - 58 us: the time is ~410 VALU + 32 MFMA issued per 64
  // queries x 64 keys (SQ_INSTS_VALU identical in every form) and ~30 % of wave cycles waiting, not the tile schedule.
  if (p.mfma != 0 && p.mfma != 16 && p.mfma != 32 && p.mfma != 64) return CV_ERR_ARG;
  if (p.waves != 0 && p.waves != 2 && p.waves != 4) return CV_ERR_ARG;
  AttnSel s;
  if (p.mfma == 64 && !p.bias && p.Tk >= 8 && p.vt_ld >= 8) {
    s.form = 64;
    s.waves = 4;
    s.lds = 3 * ATTN_STAGE_BYTES;
  } else {
    s.form = p.mfma == 32 ? 32 : 16;
    // 64-query workgroups when 128-query ones would not even fill the chip once (p.waves = 2 | 4 overrides: tuning aid)
    const int64_t wgs4 = (int64_t)p.H * ((p.Tq + 127) / 128) * p.B;
    s.waves = (p.waves == 2 || (p.waves != 4 && wgs4 < 256)) ? 2 : 4;
    s.lds = 2 * ATTN_STAGE_BYTES;
  }
  const int qpw = s.form == 64 ? 64 : 32;   // queries per wave
  s.grid_x = p.H;
  s.grid_y = (p.Tq + qpw * s.waves - 1) / (qpw * s.waves);
  s.grid_z = p.B;
  s.block = 64 * s.waves;
  *out = s;
  return CV_OK;
}
