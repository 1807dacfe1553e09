// Pair-phase and gradient-phase device code of the tiled differentiable statistics (stat_tiled.hip): HSIC and RBF-MMD, value and
// gradient, on samples of any row count.  A workgroup owns ST_TILE = 64 rows i and visits tiles of 64 partner rows j, staged with their
// squared norms by the shared tile prologue (stat_tile_device.h: st_stage, st_norms, st_stage_pair; the double sums are there too).
// Every element is the expression of the single-workgroup operators: hsic_kern_row (hsic_device.h) and mmd_pair_row (mmd_device.h) are
// hsic_kern and mmd_pair_kernel for 16 partners of one row at once, the same chains pair by pair, so the two families differ in the
// order of their sums only.  A masked pair enters every sum as an exact +0.
//
// Thread t of a tile:  row ii = t >> 2 of the tile in both phases, and
//   pair phase       partner chunk cg = t & 3: the 16 partners jj = 16 cg .. 16 cg + 15, in turn (a chain of 16 float additions);
//   gradient phase   feature residue kg = t & 3: the features k = kg, kg + 4, ... (DQ = ceil(d / 4) rounded up to 4 / 8 / 16
//                    accumulators in registers, indexed at compile time only: no scratch).  The 64 coefficients of row ii are in
//                    the registers of its four threads (16 each, from the pair phase) and reach the others through a half tile of
//                    LDS; the partners are visited in the order jj = 0 .. 63, and z_i - z_j is subtracted first, as in
//                    hsic_backward_row / mmd_backward_row.
#pragma once
#include "carel_common.h"
#include "hsic_device.h"
#include "mmd_device.h"
#include "stat_tile_device.h"

namespace carel {

constexpr int ST_CHUNK = 16;          // partners per thread of the pair phase
constexpr int ST_HALF = ST_TILE / 2;
constexpr int ST_CS = ST_HALF + 1;    // row stride of the coefficient half tile (odd)
constexpr int st_grad_xs(int dq) { return 4 * dq + 1; }      // staged row stride of the gradient kernels: their DQ features per thread, odd

// g[u] += sum over the tile's partners jj = 0 .. 63, in turn, of coef(ii, jj) * (z_i[k] - z_jj[k]), k = kg + 4 u.  All threads call.
// c: this thread's 16 coefficients of the pair phase (row ii, partners 16 cg ..); col: the partners' staged rows [64][xs];
// C: [64][ST_CS] floats of LDS, through which the coefficients of a row reach its four threads, 32 partners at a time (a loop over
// partners with its coefficient in registers would have to be unrolled 64 times: every load of the tile in flight at once).
template <int DQ>
__device__ __forceinline__ void st_grad_tile(float (&g)[DQ], const float (&zi)[DQ], const float* col, int xs, int ii, int kg, const float (&c)[ST_CHUNK],
                                             float* C) {
  for (int h = 0; h < 2; ++h) {
    __syncthreads();                             // the readers of the previous half are done
    if ((kg >> 1) == h) {
#pragma unroll
      for (int q = 0; q < ST_CHUNK; ++q) C[ii * ST_CS + (kg & 1) * ST_CHUNK + q] = c[q];
    }
    __syncthreads();
    const float* cr = C + ii * ST_CS;
    const float* zj = col + h * ST_HALF * xs + kg;
#pragma unroll 2
    for (int jj = 0; jj < ST_HALF; ++jj, zj += xs) {
      const float cv = cr[jj];
#pragma unroll
      for (int u = 0; u < DQ; ++u) g[u] = fmaf(cv, zi[u] - zj[4 * u], g[u]);
    }
  }
}

// ---- HSIC
// The (H L H) and (H K H) coefficients of one pair, as hsic_backward_row writes them: cx multiplies (x_i - x_j), cy (y_i - y_j).
__device__ __forceinline__ void st_hsic_coef(float kv, float lv, float rki, float rkj, float rli, float rlj, float tk, float tl, float fm,
                                             float inv_sx, float inv_sy, float inv, float& cx, float& cy) {
  const float lc = lv - (rli + rlj) / fm + tl / (fm * fm);       // (H L H)_ij
  const float kc = kv - (rki + rkj) / fm + tk / (fm * fm);       // (H K H)_ij
  cx = 2.0f * lc * kv * (-2.0f * inv_sx) * inv;
  cy = 2.0f * kc * lv * (-2.0f * inv_sy) * inv;
}

// ---- MMD
// the coefficient of (z_i - z_j) in d(gscale * mmd)/dz_i from the pair's signed sum_a alpha K_a, as mmd_backward_row writes it
__device__ __forceinline__ float st_mmd_coef(float dc, bool i1, bool j1, float a00, float a11, float a01, float gscale) {
  const float w = (i1 == j1) ? (i1 ? a00 : a11) : a01;
  return -4.0f * w * dc * gscale;
}

}  // namespace carel
