// The tile staging of the tiled sample-statistic kernels, stated once, with the limits and the double sums they share.  The two-block
// prologue st_stage_pair opens hsic_gram_kernel (hsic_perm.hip), ps_sweep_kernel (pdist_select.hip) and the two sums kernels of
// stat_tiled.hip; its gradient kernels stage two or three blocks with st_stage / st_norms themselves, and rbf_gram_kernel
// (mmd_perm.hip) keeps its own staging loop and norm chain (measured faster there: mmd_perm.hip).  A workgroup of ST_THREADS = 256
// threads stages ST_TILE = 64 rows i and 64 partner rows j of a sample in LDS ([64][xs], xs odd: lanes that read 16 different rows
// hit 16 different banks) and takes their squared norms, so the LDS of a workgroup does not depend on the sample size.  With
// st_stage, columns d .. xs-1 of a row and the rows past the sample's end are 0: fmaf(0, 0, dot) = dot, so a padded chain has the bits
// of the d-long one.  "The distances hsic_gram exponentiates, bit for bit" (include/carel_hip.h) holds by construction.
#pragma once
#include "carel_common.h"

namespace carel {

constexpr int STAT_MAX_ROWS = 8192;   // rows of a sample (of both samples together) every tiled statistic entry accepts
constexpr int STAT_MAX_D = 64;        // ... and its feature width
constexpr int ST_TILE = 64;
constexpr int ST_THREADS = 256;
constexpr int ST_XS = STAT_MAX_D | 1; // the widest staged row

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

// the two-block prologue: rows i0 .. -> Z[0 .. 63], rows j0 .. -> Z[64 .. 127], their 128 norms -> nrm.  One loop over the 128 d
// values (two st_stage loops measured 1 - 2 % slower in hsic_gram_kernel).  Columns d .. xs-1 are NOT written: for callers whose
// element functions read k < d only (hsic_kern, hsic_sqdist, hsic_kern_row, mmd_pair_row with xs = d | 1); others use st_stage.
template <class Row>
__device__ __forceinline__ void st_stage_pair(float* Z, float* nrm, Row row, int i0, int j0, int m, int d, int xs) {
  for (int e = threadIdx.x; e < 2 * ST_TILE * d; e += ST_THREADS) {
    const int r = e / d, k = e - r * d, g = r < ST_TILE ? i0 + r : j0 + (r - ST_TILE);
    Z[r * xs + k] = g < m ? row(g)[k] : 0.f;
  }
  __syncthreads();
  st_norms(Z, nrm, 2 * ST_TILE, d, xs);
  __syncthreads();
}

// sum of a double over the wave: a butterfly (a + b = b + a to the bit), so every lane holds the same bits
__device__ __forceinline__ double wave_sum_double(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum of a double over a workgroup of ST_THREADS in an order fixed by indices: wave_sum_double, then the four wave sums in turn.
// red: 4 doubles of LDS.  The result is valid in thread 0.
__device__ __forceinline__ double st_block_sum_double(double v, double* red) {
  v = wave_sum_double(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace carel
