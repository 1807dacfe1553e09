// The differentiable statistics on samples of up to 8192 rows: carel_hsic_tiled_fwd/bwd and carel_rbf_mmd_tiled_fwd/bwd.  The same
// numbers as carel_hsic_fwd/bwd (hsic.hip) and carel_rbf_mmd_fwd/bwd (mmd.hip), element by element the same expressions (the device
// functions of hsic_device.h / mmd_device.h are called on staged rows, stat_tiled_device.h), summed tile by tile on the whole chip
// instead of by one workgroup that holds both samples in its LDS.  Neither m x m matrix is stored.  The rows are staged and their norms
// taken by the shared tile prologue of stat_tile_device.h -- the sums kernels by st_stage_pair, the call hsic_gram_kernel and
// ps_sweep_kernel make, so a tile's K and L elements are that matrix's by construction (rbf_gram_kernel stages with a loop of its own).
//
// T = ceil(rows / 64) tiles a side.  The gradient sweeps split the T partner tiles of a row tile into S contiguous runs of `per` tiles
// (st_split: about 1024 workgroups, at most one run per tile), each run a workgroup that keeps its rows' gradient in registers.
//
// HSIC   hsic_tiled_sums_kernel    grid (T, T): K and L of one tile (the X rows, then the Y rows, through one LDS buffer); a thread adds
//                                  its 16 partners in turn, the four threads of a row by a two-level quad butterfly -> row partials
//                                  rkp / rlp [T][mp] float; sum K.L of the tile's rows in double -> part [T][T].
//        hsic_tiled_rows_kernel    RK_i, RL_i = the T partials of a row added in double in tile order, rounded once; per 256 rows the
//                                  double sums of RK_i, RL_i and RK_i RL_i (exact products), each 256 values in turn -> bpart.
//        hsic_tiled_total_kernel   one workgroup: sum K.L over the tiles, TK, TL and the cross sum in double in index order; the three-sum
//                                  value in double, rounded once.  TK, TL stay in the workspace as floats for the gradient.
//        hsic_tiled_grad_kernel    grid (S, T): per partner tile the centred coefficients of hsic_backward_row for 16 partners per
//                                  thread, then the gradient phase of stat_tiled_device.h for y and for x -> gxp / gyp [S][m][d].
//        st_grad_final_kernel      the S partials of an element added in split order.
// MMD    mmd_tiled_sums_kernel     grid (T, T): the three block sums of a tile (diagonal left out), 16 float additions per thread, then
//                                  double -> part [T][T][3].   mmd_tiled_total_kernel: one workgroup adds them in index order.
//        mmd_tiled_grad_kernel     grid (S, T), as for HSIC with the coefficient of mmd_backward_row -> gp [S][n][d]; st_grad_final_kernel.
// No atomics; every sum has an order fixed by indices, so two runs give the same bits.
#include <type_traits>
#include "stat_host.h"
#include "stat_tiled_device.h"

namespace carel {

struct StHsicArgs {
  const float* x; const float* y; long ldx, ldy;
  int m, d, T, mp, S, per;
  float inv_sx, inv_sy;
  float* out; const float* grad; float* gx; float* gy;
  double* part; double* bpart;             // [T][T], [ceil(m / 256)][3]
  float* tot; float* rk; float* rl;        // [4] (TK, TL), [mp], [mp]
  float* rkp; float* rlp;                  // [T][mp]
  float* gxp; float* gyp;                  // [S][m][d]
};

struct StMmdArgs {
  const float* s1; const float* s2; long ld1, ld2;
  MmdCfg cfg;                              // zs: the staged row stride of the kernel launched
  int T, S, per;
  float* out; const float* grad; float* g1; float* g2;
  double* part;                            // [T][T][3]
  float* gp;                               // [S][n][d]
};

// ------------------------------------------------------------------------------------------------ HSIC
__global__ __launch_bounds__(ST_THREADS) void hsic_tiled_sums_kernel(StHsicArgs a) {
  __shared__ float buf[2 * ST_TILE * ST_XS];     // rows 0..63: the tile's rows i, 64..127: its partners j
  __shared__ float nrm[2 * ST_TILE];
  __shared__ double red[4];
  const int t = threadIdx.x, ii = t >> 2, cg = t & 3, m = a.m, d = a.d, xs = d | 1;
  const int i0 = blockIdx.y * ST_TILE, j0 = blockIdx.x * ST_TILE;
  const float* x = a.x; const float* y = a.y; const long ldx = a.ldx, ldy = a.ldy;
  float kv[ST_CHUNK];
  st_stage_pair(buf, nrm, [=](int g) { return x + (long)g * ldx; }, i0, j0, m, d, xs);
  hsic_kern_row<ST_CHUNK>(buf, nrm, ii, ST_TILE + cg * ST_CHUNK, d, xs, a.inv_sx, kv);
  __syncthreads();
  st_stage_pair(buf, nrm, [=](int g) { return y + (long)g * ldy; }, i0, j0, m, d, xs);
  const bool iv = i0 + ii < m;
  float sk = 0.f, sl = 0.f, s2 = 0.f, lv[ST_CHUNK];
  hsic_kern_row<ST_CHUNK>(buf, nrm, ii, ST_TILE + cg * ST_CHUNK, d, xs, a.inv_sy, lv);
#pragma unroll
  for (int q = 0; q < ST_CHUNK; ++q)
    if (iv && j0 + cg * ST_CHUNK + q < m) { sk += kv[q]; sl += lv[q]; s2 = fmaf(kv[q], lv[q], s2); }
  sk += __shfl_xor(sk, 1, 64); sk += __shfl_xor(sk, 2, 64);
  sl += __shfl_xor(sl, 1, 64); sl += __shfl_xor(sl, 2, 64);
  s2 += __shfl_xor(s2, 1, 64); s2 += __shfl_xor(s2, 2, 64);
  if (cg == 0 && iv) {
    a.rkp[(size_t)blockIdx.x * a.mp + i0 + ii] = sk;
    a.rlp[(size_t)blockIdx.x * a.mp + i0 + ii] = sl;
  }
  const double tile = st_block_sum_double(cg == 0 ? (double)s2 : 0.0, red);
  if (t == 0) a.part[(size_t)blockIdx.y * a.T + blockIdx.x] = tile;
}

__global__ __launch_bounds__(256) void hsic_tiled_rows_kernel(StHsicArgs a) {
  __shared__ double red[3][256];
  const int t = threadIdx.x, i = blockIdx.x * 256 + t;
  float fk = 0.f, fl = 0.f;
  if (i < a.m) {
    double sk = 0.0, sl = 0.0;
    for (int q = 0; q < a.T; ++q) { sk += (double)a.rkp[(size_t)q * a.mp + i]; sl += (double)a.rlp[(size_t)q * a.mp + i]; }
    fk = (float)sk; fl = (float)sl;
    a.rk[i] = fk; a.rl[i] = fl;
  }
  red[0][t] = (double)fk; red[1][t] = (double)fl; red[2][t] = (double)fk * (double)fl;
  __syncthreads();
  if (t < 3) {
    double s = 0.0;
    for (int k = 0; k < 256; ++k) s += red[t][k];
    a.bpart[(size_t)blockIdx.x * 3 + t] = s;
  }
}

__global__ __launch_bounds__(256) void hsic_tiled_total_kernel(StHsicArgs a, int write_out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int e = t; e < a.T * a.T; e += 256) s += a.part[e];
  red[t] = s;
  __syncthreads();
  if (t == 0) {
    double slk = 0.0, tk = 0.0, tl = 0.0, cross = 0.0;
    for (int k = 0; k < 256; ++k) slk += red[k];
    const int rb = (a.m + 255) / 256;
    for (int b = 0; b < rb; ++b) { tk += a.bpart[3 * b]; tl += a.bpart[3 * b + 1]; cross += a.bpart[3 * b + 2]; }
    const double dm = (double)a.m;
    a.tot[0] = (float)tk; a.tot[1] = (float)tl;
    if (write_out) a.out[0] = (float)((slk - 2.0 / dm * cross + tk * tl / (dm * dm)) / ((dm - 1.0) * (dm - 1.0)));
  }
}

template <int DQ>
__global__ __launch_bounds__(ST_THREADS) void hsic_tiled_grad_kernel(StHsicArgs a) {
  constexpr int XS = st_grad_xs(DQ);
  __shared__ float lds[3 * ST_TILE * XS];        // the tile's X rows | the partners' rows (X, then Y, then X again) | the tile's Y rows
  __shared__ float nrm[3 * ST_TILE];             // in the same order
  __shared__ float rkc[ST_TILE], rlc[ST_TILE];   // RK, RL of the partners
  __shared__ float C[ST_TILE * ST_CS];
  float* XR = lds; float* COL = lds + ST_TILE * XS; float* YR = lds + 2 * ST_TILE * XS;
  const int t = threadIdx.x, ii = t >> 2, cg = t & 3, m = a.m, d = a.d;
  const int i0 = blockIdx.y * ST_TILE, i = i0 + ii;
  const bool iv = i < m;
  const float* x = a.x; const float* y = a.y; const long ldx = a.ldx, ldy = a.ldy;
  auto xrow = [=](int g) { return x + (long)g * ldx; };
  auto yrow = [=](int g) { return y + (long)g * ldy; };
  st_stage(XR, xrow, i0, m, d, XS);
  st_stage(YR, yrow, i0, m, d, XS);
  __syncthreads();
  st_norms(XR, nrm, ST_TILE, d, XS);
  st_norms(YR, nrm + 2 * ST_TILE, ST_TILE, d, XS);
  float xi[DQ], yi[DQ], gx[DQ], gy[DQ];
#pragma unroll
  for (int u = 0; u < DQ; ++u) { xi[u] = XR[ii * XS + cg + 4 * u]; yi[u] = YR[ii * XS + cg + 4 * u]; gx[u] = 0.f; gy[u] = 0.f; }
  const float rki = iv ? a.rk[i] : 0.f, rli = iv ? a.rl[i] : 0.f;
  const float tk = a.tot[0], tl = a.tot[1], gs = a.grad ? a.grad[0] : 1.f;
  const float fm = (float)m, inv = gs / ((fm - 1.0f) * (fm - 1.0f));
  const int tj1 = min(a.T, ((int)blockIdx.x + 1) * a.per);
  for (int tj = blockIdx.x * a.per; tj < tj1; ++tj) {
    const int j0 = tj * ST_TILE;
    __syncthreads();                             // the previous tile's gradient phase has read COL; the first tile's norms are written
    st_stage(COL, xrow, j0, m, d, XS);
    if (t < ST_TILE) { rkc[t] = j0 + t < m ? a.rk[j0 + t] : 0.f; rlc[t] = j0 + t < m ? a.rl[j0 + t] : 0.f; }
    __syncthreads();
    st_norms(COL, nrm + ST_TILE, ST_TILE, d, XS);
    __syncthreads();
    float cx[ST_CHUNK], cy[ST_CHUNK];
    hsic_kern_row<ST_CHUNK>(XR, nrm, ii, ST_TILE + cg * ST_CHUNK, d, XS, a.inv_sx, cx);      // K_ij for now
    __syncthreads();
    st_stage(COL, yrow, j0, m, d, XS);
    __syncthreads();
    st_norms(COL, nrm + ST_TILE, ST_TILE, d, XS);
    __syncthreads();
    hsic_kern_row<ST_CHUNK>(COL, nrm + ST_TILE, ST_TILE + ii, cg * ST_CHUNK, d, XS, a.inv_sy, cy);     // L_ij for now
#pragma unroll
    for (int q = 0; q < ST_CHUNK; ++q) {
      const int jj = cg * ST_CHUNK + q;
      float kv = cx[q], lv = cy[q], vx, vy;
      // (the two empty statements keep the 16 coefficient computations, two divisions each, in turn: interleaved for latency they
      // need every register the SIMD has)
      asm volatile("" : "+v"(kv), "+v"(lv));
      st_hsic_coef(kv, lv, rki, rkc[jj], rli, rlc[jj], tk, tl, fm, a.inv_sx, a.inv_sy, inv, vx, vy);
      asm volatile("" : "+v"(vx), "+v"(vy));
      const bool live = iv && j0 + jj < m;
      cx[q] = live ? vx : 0.f; cy[q] = live ? vy : 0.f;
    }
    st_grad_tile<DQ>(gy, yi, COL, XS, ii, cg, cy, C);
    __syncthreads();
    st_stage(COL, xrow, j0, m, d, XS);
    __syncthreads();
    st_grad_tile<DQ>(gx, xi, COL, XS, ii, cg, cx, C);
  }
  if (iv) {
    float* px = a.gxp + ((size_t)blockIdx.x * m + i) * d;
    float* py = a.gyp + ((size_t)blockIdx.x * m + i) * d;
#pragma unroll
    for (int u = 0; u < DQ; ++u) {
      const int k = cg + 4 * u;
      if (k < d) { px[k] = gx[u]; py[k] = gy[u]; }
    }
  }
}

// out element e = the S partials part[s][e] in turn.  Rows below n1 go to o1, the others to o2 (HSIC: two calls with n1 = rows).
__global__ __launch_bounds__(256) void st_grad_final_kernel(const float* __restrict__ part, int S, long rows, int d, long n1, float* __restrict__ o1,
                                                            float* __restrict__ o2) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x, total = rows * d;
  if (e >= total) return;
  float s = part[e];
  for (int q = 1; q < S; ++q) s += part[(size_t)q * total + e];
  if (e < n1 * d) o1[e] = s; else o2[e - n1 * d] = s;
}

// ------------------------------------------------------------------------------------------------ MMD
__global__ __launch_bounds__(ST_THREADS) void mmd_tiled_sums_kernel(StMmdArgs a) {
  __shared__ float buf[2 * ST_TILE * ST_XS];
  __shared__ float nrm[2 * ST_TILE];
  __shared__ double red[4];
  const MmdCfg& c = a.cfg;                     // zs = d | 1 (the host sets it)
  const int t = threadIdx.x, ii = t >> 2, cg = t & 3, n1 = c.n1, n = c.n1 + c.n2, d = c.d;
  const int i0 = blockIdx.y * ST_TILE, j0 = blockIdx.x * ST_TILE, i = i0 + ii;
  const float* s1 = a.s1; const float* s2 = a.s2; const long ld1 = a.ld1, ld2 = a.ld2;
  auto row = [=](int g) { return g < n1 ? s1 + (long)g * ld1 : s2 + (long)(g - n1) * ld2; };
  st_stage_pair(buf, nrm, row, i0, j0, n, d, c.zs);
  const bool i1 = i < n1;
  float s11 = 0.f, s22 = 0.f, s12 = 0.f;
  float kv[ST_CHUNK];
  mmd_pair_row<ST_CHUNK, false>(c, buf, nrm, ii, ST_TILE + cg * ST_CHUNK, kv);
#pragma unroll
  for (int q = 0; q < ST_CHUNK; ++q) {
    const int j = j0 + cg * ST_CHUNK + q;
    if (i < n && j < n && i != j) {
      const bool j1 = j < n1;
      if (i1 && j1) s11 += kv[q];
      else if (!i1 && !j1) s22 += kv[q];
      else if (i1 && !j1) s12 += kv[q];        // K12 block only (the K21 mirror is the factor 2)
    }
  }
  const double t11 = st_block_sum_double((double)s11, red);
  const double t22 = st_block_sum_double((double)s22, red);
  const double t12 = st_block_sum_double((double)s12, red);
  if (t == 0) {
    double* p = a.part + ((size_t)blockIdx.y * a.T + blockIdx.x) * 3;
    p[0] = t11; p[1] = t22; p[2] = t12;
  }
}

__global__ __launch_bounds__(256) void mmd_tiled_total_kernel(StMmdArgs a) {
  __shared__ double red[3][256];
  const int t = threadIdx.x, tiles = a.T * a.T;
  double s[3] = {0.0, 0.0, 0.0};
  for (int e = t; e < tiles; e += 256) { s[0] += a.part[3 * (size_t)e]; s[1] += a.part[3 * (size_t)e + 1]; s[2] += a.part[3 * (size_t)e + 2]; }
  red[0][t] = s[0]; red[1][t] = s[1]; red[2][t] = s[2];
  __syncthreads();
  if (t == 0) {
    double s11 = 0.0, s22 = 0.0, s12 = 0.0;
    for (int k = 0; k < 256; ++k) { s11 += red[0][k]; s22 += red[1][k]; s12 += red[2][k]; }
    const double n1 = (double)a.cfg.n1, n2 = (double)a.cfg.n2;
    const double a00 = 1.0 / (n1 * (n1 - 1.0)), a11 = 1.0 / (n2 * (n2 - 1.0)), a01 = -1.0 / (n1 * n2);
    a.out[0] = (float)(2.0 * a01 * s12 + a00 * s11 + a11 * s22);
  }
}

template <int DQ>
__global__ __launch_bounds__(ST_THREADS) void mmd_tiled_grad_kernel(StMmdArgs a) {
  constexpr int XS = st_grad_xs(DQ);
  __shared__ float lds[2 * ST_TILE * XS];        // the tile's rows | the partners' rows
  __shared__ float nrm[2 * ST_TILE];
  __shared__ float C[ST_TILE * ST_CS];
  float* COL = lds + ST_TILE * XS;
  const MmdCfg& c = a.cfg;                     // zs = XS (the host sets it)
  const int t = threadIdx.x, ii = t >> 2, cg = t & 3, n1 = c.n1, n = c.n1 + c.n2, d = c.d;
  const int i0 = blockIdx.y * ST_TILE, i = i0 + ii;
  const bool iv = i < n, i1 = i < n1;
  const float* s1 = a.s1; const float* s2 = a.s2; const long ld1 = a.ld1, ld2 = a.ld2;
  auto row = [=](int g) { return g < n1 ? s1 + (long)g * ld1 : s2 + (long)(g - n1) * ld2; };
  st_stage(lds, row, i0, n, d, XS);
  __syncthreads();
  st_norms(lds, nrm, ST_TILE, d, XS);
  float zi[DQ], g[DQ];
#pragma unroll
  for (int u = 0; u < DQ; ++u) { zi[u] = lds[ii * XS + cg + 4 * u]; g[u] = 0.f; }
  const float a00 = (float)(1.0 / ((double)c.n1 * (c.n1 - 1))), a11 = (float)(1.0 / ((double)c.n2 * (c.n2 - 1)));
  const float a01 = (float)(-1.0 / ((double)c.n1 * c.n2));
  const float gs = a.grad ? a.grad[0] : 1.0f;
  const int tj1 = min(a.T, ((int)blockIdx.x + 1) * a.per);
  for (int tj = blockIdx.x * a.per; tj < tj1; ++tj) {
    const int j0 = tj * ST_TILE;
    __syncthreads();                             // the previous tile's gradient phase has read COL
    st_stage(COL, row, j0, n, d, XS);
    __syncthreads();
    st_norms(COL, nrm + ST_TILE, ST_TILE, d, XS);
    __syncthreads();
    float cf[ST_CHUNK];
    mmd_pair_row<ST_CHUNK, true>(c, lds, nrm, ii, ST_TILE + cg * ST_CHUNK, cf);
#pragma unroll
    for (int q = 0; q < ST_CHUNK; ++q) {
      const int j = j0 + cg * ST_CHUNK + q;
      const float v = st_mmd_coef(cf[q], i1, j < n1, a00, a11, a01, gs);
      cf[q] = (iv && j < n && j != i) ? v : 0.f;
    }
    st_grad_tile<DQ>(g, zi, COL, XS, ii, cg, cf, C);
  }
  if (iv) {
    float* p = a.gp + ((size_t)blockIdx.x * n + i) * d;
#pragma unroll
    for (int u = 0; u < DQ; ++u) {
      const int k = cg + 4 * u;
      if (k < d) p[k] = g[u];
    }
  }
}

}  // namespace carel

using namespace carel;

// f(DQ as a compile-time constant) for the DQ = 4 / 8 / 16 accumulators per thread that hold a row's d features (k = kg + 4 u < 4 DQ)
template <class F>
static void st_with_dq(int d, F f) {
  if (d <= 16) f(std::integral_constant<int, 4>());
  else if (d <= 32) f(std::integral_constant<int, 8>());
  else f(std::integral_constant<int, 16>());
}

static int64_t st_tiles(int64_t rows) { return (rows + ST_TILE - 1) / ST_TILE; }

// partner tiles per gradient workgroup and the number of such runs: about 1024 workgroups, at most one run per tile
static void st_split(int T, int* per, int* S) {
  int want = 1024 / T;
  if (want < 1) want = 1;
  if (want > T) want = T;
  *per = (T + want - 1) / want;
  *S = (T + *per - 1) / *per;
}

extern "C" int64_t carel_hsic_tiled_workspace_bytes(int32_t m, int32_t d) {
  if (m < 2 || m > STAT_MAX_ROWS || d < 1 || d > STAT_MAX_D) return 0;
  const int64_t T = st_tiles(m), mp = T * ST_TILE, rb = (m + 255) / 256;
  int per, S;
  st_split((int)T, &per, &S);
  // doubles: part [T][T], bpart [rb][3]; floats: tot [4], RK [mp], RL [mp], rkp [T][mp], rlp [T][mp], gxp [S][m][d], gyp [S][m][d]
  return 8 * (T * T + 3 * rb) + 4 * (4 + 2 * mp + 2 * T * mp + 2 * (int64_t)S * m * d);
}

extern "C" int64_t carel_rbf_mmd_tiled_workspace_bytes(int32_t n1, int32_t n2, int32_t d) {
  if (n1 < 2 || n2 < 2 || (int64_t)n1 + n2 > STAT_MAX_ROWS || d < 1 || d > STAT_MAX_D) return 0;
  const int64_t n = (int64_t)n1 + n2, T = st_tiles(n);
  int per, S;
  st_split((int)T, &per, &S);
  return 8 * (3 * T * T) + 4 * ((int64_t)S * n * d);          // doubles: part [T][T][3]; floats: gp [S][n][d]
}

static int hsic_tiled_launch(const carel_hsic_args* a, void* work, int backward, hipStream_t stream, const char* who) {
  if (!a || !a->x || !a->y) return set_error(CAREL_ERR_ARG, "%s: null sample pointer", who);
  if (a->m < 2 || a->m > STAT_MAX_ROWS) return set_error(CAREL_ERR_SHAPE, "%s: m must be in 2..%d (got %d)", who, STAT_MAX_ROWS, a->m);
  if (a->d < 1 || a->d > STAT_MAX_D) return set_error(CAREL_ERR_SHAPE, "%s: d must be in 1..%d (got %d)", who, STAT_MAX_D, a->d);
  if (!(a->s_x > 0.f) || !(a->s_y > 0.f)) return set_error(CAREL_ERR_ARG, "%s: kernel widths must be positive", who);
  if (a->ldx < a->d || a->ldy < a->d) return set_error(CAREL_ERR_ARG, "%s: row stride below d", who);
  if (!backward && !a->hsic_out) return set_error(CAREL_ERR_ARG, "%s: null output", who);
  if (backward && (!a->gx || !a->gy)) return set_error(CAREL_ERR_ARG, "%s: null gradient output", who);
  if (int rc = check_workspace(who, work, 8)) return rc;
  StHsicArgs k;
  k.x = (const float*)a->x; k.y = (const float*)a->y; k.ldx = a->ldx; k.ldy = a->ldy;
  k.m = a->m; k.d = a->d; k.T = (int)st_tiles(a->m); k.mp = k.T * ST_TILE;
  st_split(k.T, &k.per, &k.S);
  k.inv_sx = 1.0f / a->s_x; k.inv_sy = 1.0f / a->s_y;
  k.out = (float*)a->hsic_out; k.grad = (const float*)a->grad_hsic; k.gx = (float*)a->gx; k.gy = (float*)a->gy;
  const int rb = (k.m + 255) / 256;
  k.part = (double*)work;
  k.bpart = k.part + (size_t)k.T * k.T;
  k.tot = (float*)(k.bpart + 3 * (size_t)rb);
  k.rk = k.tot + 4; k.rl = k.rk + k.mp;
  k.rkp = k.rl + k.mp; k.rlp = k.rkp + (size_t)k.T * k.mp;
  k.gxp = k.rlp + (size_t)k.T * k.mp; k.gyp = k.gxp + (size_t)k.S * k.m * k.d;
  hipLaunchKernelGGL(hsic_tiled_sums_kernel, dim3(k.T, k.T), dim3(ST_THREADS), 0, stream, k);
  hipLaunchKernelGGL(hsic_tiled_rows_kernel, dim3(rb), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(hsic_tiled_total_kernel, dim3(1), dim3(256), 0, stream, k, backward ? 0 : 1);
  if (backward) {
    const dim3 grid(k.S, k.T);
    st_with_dq(k.d, [&](auto dq) { hipLaunchKernelGGL(hsic_tiled_grad_kernel<dq()>, grid, dim3(ST_THREADS), 0, stream, k); });
    const long total = (long)k.m * k.d;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    hipLaunchKernelGGL(st_grad_final_kernel, dim3(blocks), dim3(256), 0, stream, (const float*)k.gxp, k.S, (long)k.m, k.d, (long)k.m, k.gx, k.gx);
    hipLaunchKernelGGL(st_grad_final_kernel, dim3(blocks), dim3(256), 0, stream, (const float*)k.gyp, k.S, (long)k.m, k.d, (long)k.m, k.gy, k.gy);
  }
  return check_launch(who);
}

extern "C" int carel_hsic_tiled_fwd(const carel_hsic_args* a, void* work, void* stream) {
  return hsic_tiled_launch(a, work, 0, (hipStream_t)stream, "carel_hsic_tiled_fwd");
}
extern "C" int carel_hsic_tiled_bwd(const carel_hsic_args* a, void* work, void* stream) {
  return hsic_tiled_launch(a, work, 1, (hipStream_t)stream, "carel_hsic_tiled_bwd");
}

static int mmd_tiled_launch(const carel_mmd_args* a, void* work, int backward, hipStream_t stream, const char* who) {
  if (!a || !a->s1 || !a->s2) return set_error(CAREL_ERR_ARG, "%s: null sample pointer", who);
  if (a->n1 < 2 || a->n2 < 2) return set_error(CAREL_ERR_SHAPE, "%s: n1,n2 must be >= 2 (the reference divides by n(n-1))", who);
  if ((int64_t)a->n1 + a->n2 > STAT_MAX_ROWS) return set_error(CAREL_ERR_SHAPE, "%s: n1 + n2 must be <= %d (got %lld)", who, STAT_MAX_ROWS, (long long)a->n1 + a->n2);
  if (a->d < 1 || a->d > STAT_MAX_D) return set_error(CAREL_ERR_SHAPE, "%s: d must be in 1..%d (got %d)", who, STAT_MAX_D, a->d);
  if (a->n_alphas < 1 || a->n_alphas > 8) return set_error(CAREL_ERR_ARG, "%s: n_alphas must be in 1..8", who);
  if (a->ld1 < a->d || a->ld2 < a->d) return set_error(CAREL_ERR_ARG, "%s: row stride below d", who);
  if (!backward && !a->mmd_out) return set_error(CAREL_ERR_ARG, "%s: null mmd_out", who);
  if (backward && (!a->g1 || !a->g2)) return set_error(CAREL_ERR_ARG, "%s: null gradient output", who);
  if (int rc = check_workspace(who, work, 8)) return rc;
  StMmdArgs k;
  k.s1 = (const float*)a->s1; k.s2 = (const float*)a->s2; k.ld1 = a->ld1; k.ld2 = a->ld2;
  fill_mmd_cfg(&k.cfg, a, a->d | 1);
  const int n = a->n1 + a->n2;
  k.T = (int)st_tiles(n);
  st_split(k.T, &k.per, &k.S);
  k.out = (float*)a->mmd_out; k.grad = (const float*)a->grad_mmd; k.g1 = (float*)a->g1; k.g2 = (float*)a->g2;
  k.part = (double*)work;
  k.gp = (float*)(k.part + 3 * (size_t)k.T * k.T);
  if (!backward) {
    hipLaunchKernelGGL(mmd_tiled_sums_kernel, dim3(k.T, k.T), dim3(ST_THREADS), 0, stream, k);
    hipLaunchKernelGGL(mmd_tiled_total_kernel, dim3(1), dim3(256), 0, stream, k);
  } else {
    const dim3 grid(k.S, k.T);
    st_with_dq(k.cfg.d, [&](auto dq) {
      k.cfg.zs = st_grad_xs(dq());               // the staged row stride of the kernel launched: its own XS
      hipLaunchKernelGGL(mmd_tiled_grad_kernel<dq()>, grid, dim3(ST_THREADS), 0, stream, k);
    });
    const long total = (long)n * k.cfg.d;
    hipLaunchKernelGGL(st_grad_final_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const float*)k.gp, k.S, (long)n, k.cfg.d,
                       (long)k.cfg.n1, k.g1, k.g2);
  }
  return check_launch(who);
}

extern "C" int carel_rbf_mmd_tiled_fwd(const carel_mmd_args* a, void* work, void* stream) {
  return mmd_tiled_launch(a, work, 0, (hipStream_t)stream, "carel_rbf_mmd_tiled_fwd");
}
extern "C" int carel_rbf_mmd_tiled_bwd(const carel_mmd_args* a, void* work, void* stream) {
  return mmd_tiled_launch(a, work, 1, (hipStream_t)stream, "carel_rbf_mmd_tiled_bwd");
}
