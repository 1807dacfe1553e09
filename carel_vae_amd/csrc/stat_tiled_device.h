// Tile-level device code of the tiled differentiable statistics (stat_tiled.hip): HSIC and RBF-MMD, value and gradient, on samples of
// any row count.  A workgroup of ST_THREADS = 256 threads owns ST_TILE = 64 rows i and visits tiles of 64 partner rows j; the rows of a
// tile and their squared norms sit in LDS ([64][xs], xs odd: lanes that read 16 different rows hit 16 different banks), so the LDS of a
// workgroup does not depend on the sample size.  Every element is the expression of the single-workgroup operators: hsic_kern_row
// (hsic_device.h) and mmd_pair_row (mmd_device.h) are hsic_kern and mmd_pair_kernel for 16 partners of one row at once, the same
// chains pair by pair, so the two families differ in the order of their sums only.  Columns d .. xs-1 of a staged row and the rows past the sample's end are 0: fmaf(0, 0, dot) = dot, so
// the padded chains have the bits of the d-long ones, and a masked pair enters every sum as an exact +0.
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

namespace carel {

constexpr int ST_TILE = 64;
constexpr int ST_THREADS = 256;
constexpr int ST_CHUNK = 16;          // partners per thread of the pair phase

// rows r0 .. r0 + 63 of a sample -> dst[64][xs]; row(g) is the address of row g; rows >= m and the columns d .. xs-1 are 0
template <class Row>
__device__ __forceinline__ void st_stage(float* dst, Row row, int r0, int m, int d, int xs) {
  for (int e = threadIdx.x; e < ST_TILE * xs; e += ST_THREADS) {
    const int r = e / xs, k = e - r * xs, g = r0 + r;
    dst[e] = (g < m && k < d) ? row(g)[k] : 0.f;
  }
}

// squared norms of `rows` staged rows by the chain of hsic_forward_block / mmd_forward_block (threads 0 .. rows-1)
__device__ __forceinline__ void st_norms(const float* Z, float* nrm, int rows, int d, int xs) {
  if ((int)threadIdx.x < rows) {
    const float* z = Z + threadIdx.x * xs;
    float s = 0.f;
    for (int k = 0; k < d; ++k) s = fmaf(z[k], z[k], s);
    nrm[threadIdx.x] = s;
  }
}

constexpr int ST_HALF = ST_TILE / 2;
constexpr int ST_CS = ST_HALF + 1;    // row stride of the coefficient half tile (odd)

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

// sum of a double over the workgroup in an order fixed by indices: butterfly within the wave (a + b = b + a to the bit), the four wave
// sums in turn.  red: 4 doubles of LDS.  The result is valid in thread 0.
__device__ __forceinline__ double st_block_sum_double(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
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
