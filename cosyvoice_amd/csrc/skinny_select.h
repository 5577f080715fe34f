// cv_skinny_gemm, steps one and two of three: check the parameter block, then pick the kernel form, grid and LDS size.  Plain C++17 over
// the public header only (no HIP), so the host compiler alone builds it and tests/test_skinny_select_cpu.py holds every pick to the
// recorded ones.  Step three, turning a SkinnySel into the template instantiation and launching it, is launch_skinny in llm.hip.
#pragma once
#include <stddef.h>
#include "../../include/cosyvoice_amd.h"

// skinny_kernel<DT, TPW, NORM, TPR, U, RS, MR> (single-shot) or skinny_stream_kernel<DT, TPW, NORM, TPR, U>; block = 256 threads
struct SkinnySel {
  bool stream;       // workgroups walk several tile groups with the next group's weights in flight (grid_x < tile groups)
  int tpw;           // 16-column tiles per workgroup: 2 = the (gate, up) pair of mode 2 or the long-K two-row-group form
  int norm;          // 0 = A from memory, 1 + n_nslab = fused RMSNorm prologue
  int tpr;           // threads per activation row in that prologue (16 without one)
  int u;             // weight fragments a wave keeps in flight per tile
  bool rs;           // consumer half of the split RMSNorm (rs_part)
  int mr;            // 16-row groups of activation rows
  unsigned grid_x, grid_y;
  size_t lds;
};

// The forms the library builds: 54 single-shot + 28 streaming per dtype.  launch_skinny instantiates exactly these.
constexpr bool skinny_built(bool stream, int tpw, int norm, int tpr, int u, bool rs, int mr) {
  if (tpw != 1 && tpw != 2) return false;
  if (mr == 2)   // two row groups: single-shot, plain rows
    return !stream && norm == 0 && tpr == 16 && (tpw == 1 ? !rs && (u == 7 || u == 8 || u == 12 || u == 16) : (rs ? u == 7 || u == 8 : u == 10));
  if (mr != 1) return false;
  if (rs) return !stream && tpw == 2 && norm == 0 && tpr == 16 && (u == 7 || u == 8);
  if (norm == 0) return tpr == 16 && (tpw == 1 ? u == 8 || u == 12 || u == 16 || (u == 7 && !stream) : u == 8);
  return (norm == 1 || norm == 2 || norm == 3 || norm == 5) && (tpr == 16 || tpr == 32 || tpr == 64) &&
         (u == 8 || (u == 7 && !stream && tpr != 64));
}

// Checks and defaults (written back into p: ksplit <= 0 -> 1, max_wgs = 0 where only single-shot forms exist), then the pick.
// Returns CV_OK and fills *out, or the status code cv_skinny_gemm returns.  p.dtype is the launcher's to check.
inline int skinny_select(cv_skinny_params& p, SkinnySel* out) {
  const bool norm = p.ngamma != nullptr;
  if (p.M <= 0 || p.M > 32 || p.N <= 0 || p.K <= 0 || (p.K & 31) || !p.Wp) return CV_ERR_ARG;
  if (p.M > 16 && (norm || p.mode == 3)) return CV_ERR_UNSUPPORTED;   // two row groups: plain-row forms of modes 0 / 1 / 2 only
  if (!norm && (!p.A || (p.lda & 7))) return CV_ERR_ARG;
  if (norm) {
    if (!p.nx || (p.K & 63) || p.K > 1024 || (p.ldnx & 3) || p.nx_out == p.nx) return CV_ERR_ARG;
    if (p.n_nslab > 0 && (!p.nslabs || (p.ld_nslab & 3) || (p.nslab_stride & 3))) return CV_ERR_ARG;
    if (p.n_nslab != 0 && p.n_nslab != 1 && p.n_nslab != 2 && p.n_nslab != 4) return CV_ERR_ARG;
  }
  if (p.ksplit <= 0) p.ksplit = 1;
  const int ntiles = (p.N + 15) / 16, nks = p.K >> 5;
  if (p.mode == 2) {
    if (p.ksplit != 1 || (ntiles & 1) || !p.out_act || (p.ldoa & 3)) return CV_ERR_ARG;
    if (p.rs_part) {
      if (norm || p.n_rs_part <= 0 || p.n_rs_part > 64) return CV_ERR_ARG;
      p.max_wgs = 0;
    }
  } else if (p.mode == 3) {
    if (p.ksplit != 1 || !p.out_act || norm) return CV_ERR_ARG;
    p.max_wgs = 0;   // single-shot kernel only
  } else if (p.mode == 1 && (p.xb_out || p.ss_part)) {
    if (!p.out_f32 || p.ksplit != 1 || !p.xb_out || !p.ss_part || p.ldxb < p.N) return CV_ERR_ARG;
    p.max_wgs = 0;
  } else {
    if (!p.out_f32) return CV_ERR_ARG;
    if (p.mode == 1 && p.ksplit != 1) return CV_ERR_ARG;
  }
  // k-steps one wave covers: the streaming kernel takes them as one batch of U fragment loads
  const int per_wave = (((nks + p.ksplit - 1) / p.ksplit) + 3) >> 2;
  if (p.mode == 2 && p.rs_part && per_wave > 8) return CV_ERR_UNSUPPORTED;   // split-norm consumer: K <= 1024 only

  SkinnySel s;
  s.stream = false;
  s.tpw = p.mode == 2 ? 2 : 1;
  s.norm = norm ? 1 + p.n_nslab : 0;
  s.tpr = !norm ? 16 : (p.M <= 4 ? 64 : (p.M <= 8 ? 32 : 16));
  s.rs = p.mode == 2 && p.rs_part;
  s.mr = p.M > 16 ? 2 : 1;
  const int ngroups = ntiles / s.tpw;
  s.grid_x = ngroups;
  s.grid_y = p.ksplit;
  const int u_plain = per_wave <= 8 ? 8 : (per_wave <= 12 ? 12 : 16);
  // every wave's K slice is exactly 7 k-steps (K = 896 * ksplit): single-shot launches use the clamp-free U = 7 form
  bool exact7 = per_wave == 7 && nks == 28 * p.ksplit;
  if (s.mr == 2) {   // 17..32 rows: two 16-row groups share every weight fragment; single-shot workgroups
    if (s.tpw == 2) {
      if (!p.rs_part) return CV_ERR_UNSUPPORTED;
      // (two (gate, up) tile pairs per workgroup — skinny_kernel<DT, 4, 0, 16, 7, true, 2>, half the activation traffic — was measured at
      // 19.9 vs 20.7 us on 64 CUs and 10.8 vs 10.4 us on all: at 240 VGPRs its 152 workgroups still need two rounds; not dispatched)
      s.u = exact7 ? 7 : 8;
    } else if (per_wave > 8 && per_wave <= 10 && !(ntiles & 1)) {
      // long-K form (the down projection): with two row groups the activation slice a workgroup reads (32 rows x its K range) is twice
      // its weight tile, so two weight tiles share it (TPW = 2: half the workgroups, half the activation traffic)
      s.tpw = 2;
      s.grid_x = ngroups / 2;
      s.u = 10;
    } else {
      s.u = exact7 ? 7 : u_plain;
    }
  } else if (per_wave > 16 || (s.tpw == 2 && per_wave > 8)) {
    // slices longer than one batch of loads: the single-shot kernel loops over them (plain rows: the prologue's K <= 1024 is per_wave <= 8)
    s.u = 8;
  } else {
    if (p.max_wgs > 0) {
      const int cap = p.max_wgs / p.ksplit;
      s.grid_x = ngroups < cap ? ngroups : (cap > 1 ? cap : 1);
    }
    s.stream = (int)s.grid_x < ngroups;
    exact7 = exact7 && !s.stream;
    // U = 7 exists where the VGPR diet needs it (llm.hip, skinny_kernel): not for the TPR = 64 prologue, nor the plain gate/up form
    if (s.norm != 0 ? s.tpr == 64 : (s.tpw == 2 && !s.rs)) exact7 = false;
    s.u = exact7 ? 7 : u_plain;
  }
  const size_t red = (size_t)4 * s.tpw * 64 * 4 * sizeof(float);            // [4 waves][tpw][64 lanes] float4 per row group / buffer
  s.lds = (s.stream ? 2 : s.mr) * red + (norm ? (size_t)nks * 1024 : 0);     // + the prologue's fragment image
  *out = s;
  return CV_OK;
}
