// The permutation independence test on the HSIC statistic (Gretton et al. 2007) and the tiled Gram matrix it is run on.  The reference
// has no such function: the definition is this project's own (include/carel_hip.h, parity unpinned); the statistic is the reference's
// HSIC, tr(L H K H) / (m-1)^2 (drl_classifier_ec_hsic.py:540-547).
//
// carel_hsic_perm_test.  stat(pi) = sum_ij Kc_ij L[pi_i][pi_j] / (m-1)^2 with Kc = H K H.
//   hsic_pack_kernel     perms i32 -> idx u16 [P+1][m4] (m4 = m rounded up to 4), every index clamped into [0, m) HERE: nothing after it
//                        reads `perms`, so nothing after it can address outside a matrix.  The columns past m hold index 0.
//   hsic_rowsum_kernel   R_i in double: a wave per row, a lane adds every 64th element in turn, then a butterfly (a + b = b + a bitwise).
//   hsic_colpart_kernel  the column sums of 64 rows in double, a thread per column; hsic_colsum_kernel adds the 64-row parts in turn
//                        (C_j) and, in its last workgroup, T from the R_i.
//   hsic_centre_kernel   Kc_ij = (float)(K_ij - R_i/m - C_j/m + T/m^2), formed in double, rounded once; [m][m4], the columns past m are 0.
//                        The statistic is NOT taken by the three-sum expansion: at m = 8 192 that is a small difference of large sums.
//   hsic_gather_kernel   a workgroup owns HG_SLAB rows i and G permutations.  Per row it stages row pi_i of L for each of its
//                        permutations in LDS (coalesced), reads Kc[i][.] once (float4), gathers L[pi_i][pi_j] from LDS -- a few
//                        bank-conflict cycles per wave instead of 64 cache lines -- and accumulates fma((double)kc, (double)l, acc):
//                        the product is exact, no f32 sum exists.  A thread keeps its own pi_j in registers (four u16 per
//                        1024-column block, loaded once for the slab) and carries the NEXT row's L values in registers: they are
//                        loaded before this row's gathers and stored to LDS in the next pass, so a row costs no exposed global
//                        latency (measured: 3.69 -> 2.46 ms at m = 1 938, P = 1 000; the registers alone, without the row-ahead
//                        loads, lost a wave per SIMD and were slower, 3.87 ms).  A lane's order is (row, column block); lanes by
//                        butterfly, the four waves in turn -> part[slab][P+1].  G = 4 while four rows of L fit 48 KB (m <= HG_M4 =
//                        3072: the Kc row and its conversion are shared by four permutations), else 1 (32 KB at 8 192).
//   hsic_stats_kernel    adds the slabs in turn and divides; perm_count (the count kernel of mmd_perm.hip, the same kernel for both
//                        tests) compares the doubles and counts (integers).
// No atomics, no host synchronisation; a permutation has the same bits in whatever row of `perms` it stands (every slot of a group
// runs the same instructions in the same order) and on every run.
//
// carel_hsic_gram.  64 x 64 tiles; the 64 + 64 sample rows of a tile and their squared norms are staged by the shared prologue
// (st_stage_pair of stat_tile_device.h: 33 KB of LDS whatever m is; ps_sweep_kernel makes the same call, so its distances are these by
// construction) and every element is hsic_kern of hsic_device.h, symmetric in its two rows; on the diagonal dot is the norm's own
// chain, so the argument is -0.
#include "carel_hip_internal.h"
#include "hsic_device.h"
#include "stat_tile_device.h"

namespace carel {

constexpr int HP_MAX_P = 65535;
constexpr int HG_SLAB = 64;      // rows i per workgroup of the gather kernel (tests/hsic_perm_restate.py: SLAB)
constexpr int HG_M4 = 3072;      // four staged rows of L up to here (48 KB), one above (GROUP_M)
constexpr int HC_ROWS = 64;      // rows per column-sum part

struct HsicPermArgs {
  const float* K; long ldk;
  const float* L; long ldl;
  const int* perms;              // [np1][m]
  int m, m4, np1;
  float* kc;                     // [m][m4]
  unsigned short* idx;           // [np1][m4]
  double* part;                  // [slabs][np1]
  double* rsum; double* csum; double* tot;   // [m], [m], [1]
  double* colpart;               // [ceil(m / HC_ROWS)][m]
};

__global__ __launch_bounds__(256) void hsic_pack_kernel(HsicPermArgs a) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)a.np1 * a.m4) return;
  const int p = (int)(e / a.m4), c = (int)(e - (long)p * a.m4);
  int v = 0;
  if (c < a.m) {
    v = a.perms[(long)p * a.m + c];
    v = v < 0 ? 0 : (v >= a.m ? a.m - 1 : v);
  }
  a.idx[e] = (unsigned short)v;
}

__global__ __launch_bounds__(256) void hsic_rowsum_kernel(HsicPermArgs a) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.m) return;                      // (whole waves leave: the shuffles below see full waves)
  const float* row = a.K + (long)i * a.ldk;
  double s = 0.0;
  for (int j = lane; j < a.m; j += 64) s += (double)row[j];
  s = wave_sum_double(s);
  if (lane == 0) a.rsum[i] = s;
}

__global__ __launch_bounds__(256) void hsic_colpart_kernel(HsicPermArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.m) return;
  const int i0 = blockIdx.y * HC_ROWS, i1 = min(i0 + HC_ROWS, a.m);
  double s = 0.0;
  for (int i = i0; i < i1; ++i) s += (double)a.K[(long)i * a.ldk + j];
  a.colpart[(long)blockIdx.y * a.m + j] = s;
}

__global__ __launch_bounds__(256) void hsic_colsum_kernel(HsicPermArgs a, int parts) {
  __shared__ double red[256];
  if (blockIdx.x + 1 == gridDim.x) {         // the last workgroup: T = sum_i R_i, every 256th in turn, then the 256 partial sums in turn
    double s = 0.0;
    for (int i = threadIdx.x; i < a.m; i += 256) s += a.rsum[i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int k = 0; k < 256; ++k) t += red[k];
      a.tot[0] = t;
    }
    return;
  }
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.m) return;
  double s = 0.0;
  for (int q = 0; q < parts; ++q) s += a.colpart[(long)q * a.m + j];
  a.csum[j] = s;
}

__global__ __launch_bounds__(256) void hsic_centre_kernel(HsicPermArgs a) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)a.m * a.m4) return;
  const int i = (int)(e / a.m4), c = (int)(e - (long)i * a.m4);
  float v = 0.f;
  if (c < a.m) {
    const double dm = (double)a.m;
    v = (float)((((double)a.K[(long)i * a.ldk + c] - a.rsum[i] / dm) - a.csum[c] / dm) + a.tot[0] / (dm * dm));
  }
  a.kc[e] = v;
}

template <int G>
__global__ __launch_bounds__(256) void hsic_gather_kernel(HsicPermArgs a) {
  extern __shared__ float Lrow[];            // [G][m4]: row pi_i of L for each permutation of the group
  __shared__ double red[4 * G];
  __shared__ unsigned short rix[G * HG_SLAB];    // pi_i of the slab's rows
  const int t = threadIdx.x, m = a.m, m4 = a.m4;
  const int i0 = blockIdx.y * HG_SLAB, i1 = min(i0 + HG_SLAB, m);
  const int p0 = blockIdx.x * G;
  constexpr int MAXM = G == 4 ? HG_M4 : STAT_MAX_ROWS;
  constexpr int TRIPS = MAXM / 1024;         // column blocks of 1024 a thread visits: 3 / 8
  constexpr int TS = MAXM / 256;             // floats of a staged row a thread carries: 12 / 32
  uint2 w[G][TRIPS];                         // this thread's pi_j, four u16 per column block, loaded ONCE for the slab's rows
  float v[G][TS];                            // the NEXT row's L values on their way global -> registers -> LDS
  float4 k4[TRIPS];
  double acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {              // (a slot past the last permutation computes the last one again and writes nothing)
    const unsigned short* idx = a.idx + (size_t)min(p0 + g, a.np1 - 1) * m4;
    acc[g] = 0.0;
#pragma unroll
    for (int q = 0; q < TRIPS; ++q) {
      const int c = 4 * t + 1024 * q;
      w[g][q] = c < m4 ? *reinterpret_cast<const uint2*>(idx + c) : make_uint2(0u, 0u);
    }
    if (t < HG_SLAB) rix[g * HG_SLAB + t] = idx[min(i0 + t, m - 1)];
  }
  __syncthreads();
  // A row's operands are loaded a row ahead: the loads of row i + 1 are issued before the gathers of row i and first touched when the
  // next pass stores them to LDS, so their latency lies under the arithmetic (and under the other workgroups of the CU).
  auto fetch = [&](int i) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float* src = a.L + (long)rix[g * HG_SLAB + (i - i0)] * a.ldl;
#pragma unroll
      for (int q = 0; q < TS; ++q) {
        const int c = t + 256 * q;
        if (c < m) v[g][q] = src[c];
      }
    }
  };
  fetch(i0);
  for (int i = i0; i < i1; ++i) {
    const float* kc = a.kc + (size_t)i * m4;
#pragma unroll
    for (int q = 0; q < TRIPS; ++q) {
      const int c = 4 * t + 1024 * q;
      if (c < m4) k4[q] = *reinterpret_cast<const float4*>(kc + c);
    }
    __syncthreads();                         // the previous row's gathers are done
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int q = 0; q < TS; ++q) {
        const int c = t + 256 * q;
        if (c < m) Lrow[g * m4 + c] = v[g][q];
      }
    }
    __syncthreads();
    if (i + 1 < i1) fetch(i + 1);
#pragma unroll
    for (int q = 0; q < TRIPS; ++q) {
      const int c = 4 * t + 1024 * q;
      if (c < m4) {
        const double k0 = (double)k4[q].x, k1 = (double)k4[q].y, k2 = (double)k4[q].z, k3 = (double)k4[q].w;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float* lr = Lrow + g * m4;
          acc[g] = fma(k0, (double)lr[w[g][q].x & 0xffffu], acc[g]);
          acc[g] = fma(k1, (double)lr[w[g][q].x >> 16], acc[g]);
          acc[g] = fma(k2, (double)lr[w[g][q].y & 0xffffu], acc[g]);
          acc[g] = fma(k3, (double)lr[w[g][q].y >> 16], acc[g]);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const double v = wave_sum_double(acc[g]);
    if ((t & 63) == 0) red[(t >> 6) * G + g] = v;
  }
  __syncthreads();
  if (t < G && p0 + t < a.np1) a.part[(size_t)blockIdx.y * a.np1 + p0 + t] = ((red[t] + red[G + t]) + red[2 * G + t]) + red[3 * G + t];
}

__global__ __launch_bounds__(256) void hsic_stats_kernel(const double* __restrict__ part, int slabs, int np1, double den, double* __restrict__ stats) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= np1) return;
  double s = 0.0;
  for (int q = 0; q < slabs; ++q) s += part[(size_t)q * np1 + p];
  stats[p] = s / den;
}

// ---- the Gram matrix of one sample, tiled
struct HsicGramArgs { const float* x; long ldx; int m, d, xs; float inv_s; float* out; long ldk; };

__global__ __launch_bounds__(ST_THREADS) void hsic_gram_kernel(HsicGramArgs a) {
  __shared__ float X[2 * ST_TILE * ST_XS];   // rows 0..63: the tile's rows i, 64..127: its columns j; row stride xs = d | 1
  __shared__ float nrm[2 * ST_TILE];
  const int t = threadIdx.x, m = a.m, d = a.d, xs = a.xs;
  const int i0 = blockIdx.y * ST_TILE, j0 = blockIdx.x * ST_TILE;
  const float* x = a.x; const long ldx = a.ldx;
  st_stage_pair(X, nrm, [=](int g) { return x + (long)g * ldx; }, i0, j0, m, d, xs);
  for (int e = t; e < ST_TILE * ST_TILE; e += ST_THREADS) {
    const int ii = e / ST_TILE, jj = e - ii * ST_TILE;
    if (i0 + ii < m && j0 + jj < m) a.out[(long)(i0 + ii) * a.ldk + (j0 + jj)] = hsic_kern(X, nrm, ii, ST_TILE + jj, d, xs, a.inv_s);
  }
}

}  // namespace carel

using namespace carel;

static int64_t hp_slabs(int64_t m) { return (m + HG_SLAB - 1) / HG_SLAB; }
static int64_t hp_colparts(int64_t m) { return (m + HC_ROWS - 1) / HC_ROWS; }
static int64_t hp_m4(int64_t m) { return (m + 3) & ~(int64_t)3; }

extern "C" int64_t carel_hsic_perm_workspace_bytes(int32_t m, int32_t n_permutations) {
  if (m < 2 || m > STAT_MAX_ROWS || n_permutations < 1 || n_permutations > HP_MAX_P) return 0;
  const int64_t np1 = (int64_t)n_permutations + 1, m4 = hp_m4(m);
  // Kc f32 [m][m4], idx u16 [P+1][m4], then the doubles: part [slabs][P+1], R [m], C [m], T [1], the column-sum parts [parts][m]
  return 4 * (int64_t)m * m4 + 2 * np1 * m4 + 8 * (hp_slabs(m) * np1 + 2 * (int64_t)m + 1 + hp_colparts(m) * m);
}

extern "C" int carel_hsic_perm_test(const carel_hsic_perm_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "carel_hsic_perm_test";
  if (!a || !a->k || !a->l || !a->perms || !a->stats || !a->count || !a->workspace) return set_error(CAREL_ERR_ARG, "%s: null pointer", who);
  if (a->m < 2 || a->m > STAT_MAX_ROWS) return set_error(CAREL_ERR_SHAPE, "%s: m must be in 2..%d (got %d)", who, STAT_MAX_ROWS, a->m);
  if (a->n_permutations < 1 || a->n_permutations > HP_MAX_P)
    return set_error(CAREL_ERR_SHAPE, "%s: n_permutations must be in 1..%d (got %d)", who, HP_MAX_P, a->n_permutations);
  if (a->ldk < a->m || a->ldl < a->m)
    return set_error(CAREL_ERR_ARG, "%s: row strides %lld, %lld below m = %d", who, (long long)a->ldk, (long long)a->ldl, a->m);
  if (int rc = check_workspace(who, a->workspace, 16, a->workspace_bytes, carel_hsic_perm_workspace_bytes(a->m, a->n_permutations))) return rc;
  HsicPermArgs k;
  k.K = (const float*)a->k; k.ldk = a->ldk; k.L = (const float*)a->l; k.ldl = a->ldl; k.perms = (const int*)a->perms;
  k.m = a->m; k.m4 = (int)hp_m4(a->m); k.np1 = a->n_permutations + 1;
  const int slabs = (int)hp_slabs(k.m), parts = (int)hp_colparts(k.m);
  k.kc = (float*)a->workspace;
  k.idx = (unsigned short*)(k.kc + (size_t)k.m * k.m4);
  k.part = (double*)(k.idx + (size_t)k.np1 * k.m4);
  k.rsum = k.part + (size_t)slabs * k.np1;
  k.csum = k.rsum + k.m;
  k.tot = k.csum + k.m;
  k.colpart = k.tot + 1;
  const unsigned colblocks = (unsigned)((k.m + 255) / 256);
  hipLaunchKernelGGL(hsic_pack_kernel, dim3((unsigned)(((long)k.np1 * k.m4 + 255) / 256)), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(hsic_rowsum_kernel, dim3((unsigned)((k.m + 3) / 4)), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(hsic_colpart_kernel, dim3(colblocks, (unsigned)parts), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(hsic_colsum_kernel, dim3(colblocks + 1), dim3(256), 0, stream, k, parts);
  hipLaunchKernelGGL(hsic_centre_kernel, dim3((unsigned)(((long)k.m * k.m4 + 255) / 256)), dim3(256), 0, stream, k);
  if (k.m <= HG_M4)
    hipLaunchKernelGGL(hsic_gather_kernel<4>, dim3((unsigned)((k.np1 + 3) / 4), (unsigned)slabs), dim3(256), (size_t)4 * k.m4 * sizeof(float), stream, k);
  else
    hipLaunchKernelGGL(hsic_gather_kernel<1>, dim3((unsigned)k.np1, (unsigned)slabs), dim3(256), (size_t)k.m4 * sizeof(float), stream, k);
  const double m1 = (double)(k.m - 1);
  hipLaunchKernelGGL(hsic_stats_kernel, dim3((unsigned)((k.np1 + 255) / 256)), dim3(256), 0, stream, (const double*)k.part, slabs, k.np1, m1 * m1,
                     (double*)a->stats);
  perm_count((const double*)a->stats, k.np1, (int*)a->count, stream);
  return check_launch("carel_hsic_perm_test");
}

extern "C" int carel_hsic_gram(const carel_hsic_gram_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "carel_hsic_gram";
  if (!a || !a->x || !a->k_out) return set_error(CAREL_ERR_ARG, "%s: null pointer", who);
  if (a->m < 2 || a->m > STAT_MAX_ROWS) return set_error(CAREL_ERR_SHAPE, "%s: m must be in 2..%d (got %d)", who, STAT_MAX_ROWS, a->m);
  if (a->d < 1 || a->d > STAT_MAX_D) return set_error(CAREL_ERR_SHAPE, "%s: d must be in 1..%d (got %d)", who, STAT_MAX_D, a->d);
  if (!(a->s > 0.f)) return set_error(CAREL_ERR_ARG, "%s: the kernel width must be positive", who);
  if (a->ldx < a->d) return set_error(CAREL_ERR_ARG, "%s: row stride of x below d", who);
  if (a->ldk < a->m) return set_error(CAREL_ERR_ARG, "%s: row stride of k_out below m", who);
  HsicGramArgs k;
  k.x = (const float*)a->x; k.ldx = a->ldx; k.m = a->m; k.d = a->d; k.xs = a->d | 1; k.inv_s = 1.0f / a->s; k.out = (float*)a->k_out; k.ldk = a->ldk;
  const int tiles = (k.m + ST_TILE - 1) / ST_TILE;
  hipLaunchKernelGGL(hsic_gram_kernel, dim3(tiles, tiles), dim3(ST_THREADS), 0, stream, k);
  return check_launch("carel_hsic_gram");
}
