// The permutation two-sample test behind MMDStatistic.pval (the reference's permutation_test_mat is a stub, :599-600; the definition
// is this project's own, include/carel_hip.h), the tiled RBF Gram matrix it is run on, and the sampled latents of a pair_latents block.
//
// carel_mmd_perm_test.  With S = M' + M'^T (M' = M without its diagonal; one f32 addition per element, bitwise symmetric) and a
// labelling g, the three sums of the statistic are
//     2 S11 = sum_{i: g_i = 1} Y1[i],   S01 = sum_{i: g_i = 1} Y0[i],   2 S00 = sum_{i: g_i = 0} Y0[i],
//     Y1[i] = sum_j S_ij g_j,           Y0[i] = sum_j S_ij (1 - g_j),
// all of them sums of terms of one sign for a kernel matrix: nothing is obtained as a difference of larger sums, so the error of a
// statistic is that of its own three sums.  Y1 and Y0 are [n, n] x [n, P+1] products with 0 / 1 on the right, run on the exact f32
// MFMA (v_mfma_f32_32x32x2_f32: per output a k-ordered fmaf chain).  perm_tile_kernel: a workgroup owns 32 rows x 128 labellings (a
// wave 32 x 32); j runs in chunks of PT_CHUNK, the matrix tiles through LDS.  After each chunk the two accumulator tiles are converted to double, split
// by the row's own label and added to three double sums per lane, rows in register order; the accumulators restart at zero.  So an
// f32 chain is never longer than PT_CHUNK, everything after it is double, and every order is fixed by indices: a labelling gets the
// same bits wherever it stands in `labels` and on every run.  The two lane halves (rows 4h + ...) are added once at the end; the
// workgroup's sums go to part[row tile][3][P+1], perm_stats_kernel adds the row tiles in turn and forms stats, perm_count_kernel
// compares the doubles and counts (integers; perm_count: the HSIC test of hsic_perm.hip ends with the same kernel).  perm_pack_kernel
// first turns the label bytes into one 32-bit word per labelling and chunk, so a lane of the tile kernel loads its labelling's 32
// partners as one word.  No atomics, no host synchronisation.
//
// carel_rbf_gram.  64 x 64 tiles; the 64 + 64 sample rows of a tile and their squared norms sit in LDS (33 KB whatever n is) and every
// element is mmd_pair_kernel of mmd_device.h, whose arithmetic is symmetric in its two rows: out[i][j] and out[j][i] have the same bits.
// The tile, the thread count and the limits are those of stat_tile_device.h; the staging loop and the norm chain are this kernel's
// own, NOT st_stage_pair: with the two-sample row lambda the shared loop selects base pointer and stride per element and measured
// 1 % slower (0.0627 -> 0.0634 ms at n = 3 876, d = 24), while this loop branches per sample with scalar strides.  Same values, same
// places, the same k-ascending fmaf chain as st_norms.
#include "stat_host.h"
#include "stat_tile_device.h"
#include "tail_device.h"

namespace carel {

constexpr int PT_ROWS = 32;      // matrix rows per workgroup: one MFMA tile
constexpr int PT_LABS = 128;     // labellings per workgroup: 32 per wave
constexpr int PT_CHUNK = 32;     // partners j per f32 chain (tests/perm_restate.py: CHUNK)
constexpr int PT_LD = 33;        // LDS row stride in floats: rows 33 apart and the two k of a step 1 apart fall into different banks
constexpr int PERM_MAX_P = 65535;
static_assert(PT_ROWS == 32 && PT_CHUNK == PT_ROWS && PT_CHUNK % 2 == 0, "one staging loop fills both matrix tiles");

struct PermArgs {
  const float* M; long ldm;
  const unsigned char* labels;   // [np1, n]
  int n, np1;                    // np1 = P + 1 labellings
  double* part;                  // [tiles][3][np1]: 2 S00, 2 S11, S01 of the tile's rows
  unsigned* bits;                // [tiles][np1]: bit b of word (q, p) = label (p, 32 q + b) != 0, 0 past n
};

// labels as one 32-bit word per labelling and chunk: the tile kernel then loads ONE word per lane and chunk instead of 32 bytes
__global__ __launch_bounds__(256) void perm_pack_kernel(PermArgs a, int nchunk) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)nchunk * a.np1) return;
  const int p = (int)(e / nchunk), q = (int)(e - (long)p * nchunk);       // the chunk runs fastest: a wave reads 2 KB of one row
  const unsigned char* row = a.labels + (long)p * a.n;
  unsigned char v[PT_CHUNK];
#pragma unroll
  for (int b = 0; b < PT_CHUNK; ++b) v[b] = row[q * PT_CHUNK + b < a.n ? q * PT_CHUNK + b : 0];
  unsigned w = 0;
#pragma unroll
  for (int b = 0; b < PT_CHUNK; ++b) w |= (q * PT_CHUNK + b < a.n && v[b]) ? 1u << b : 0u;
  a.bits[(size_t)q * a.np1 + p] = w;
}

__global__ __launch_bounds__(256) void perm_tile_kernel(PermArgs a) {
  __shared__ float As[PT_ROWS * PT_LD];      // [r][c] = M[i0 + r][j0 + c]
  __shared__ float At[PT_CHUNK * PT_LD];     // [c][r] = M[j0 + c][i0 + r]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int n = a.n, np1 = a.np1;
  const int tile = blockIdx.x;
  const int i0 = tile * PT_ROWS, p0 = blockIdx.y * PT_LABS;
  const int p = p0 + wave * 32 + col;        // this lane's labelling: column `col` of the wave's output tile
  const bool plive = p < np1;
  const int pc = plive ? p : 0;              // (a lane past the last labelling computes labelling 0 again and writes nothing)
  unsigned rowmask = 0;                      // bit r: the label of the row that accumulator register r holds
  {
    const unsigned w = a.bits[(size_t)tile * np1 + pc];     // PT_ROWS == PT_CHUNK: the tile's rows are chunk `tile`
#pragma unroll
    for (int r = 0; r < 16; ++r) rowmask |= ((w >> acc32_row(r, lane)) & 1u) << r;
  }
  double s00 = 0.0, s11 = 0.0, s01 = 0.0;
  const int c = t & 31, r8 = t >> 5;
  // A chunk's operands go global -> registers -> LDS (the labels: one word, straight to its lane).  The next chunk's loads are issued
  // before this chunk's MFMAs and are not touched until the next pass stores them, so they land under the arithmetic.  Every load is
  // unconditional -- from element 0 where the index is outside -- and masked when it is stored: the loads then issue back to back.
  float va[PT_ROWS / 8], vt[PT_ROWS / 8];
  unsigned wnext;
  auto fetch = [&](int j0) {
    const bool jc = j0 + c < n, ic = i0 + c < n;
#pragma unroll
    for (int q = 0; q < PT_ROWS / 8; ++q) {
      const int r = r8 + 8 * q;
      va[q] = a.M[(i0 + r < n && jc) ? (long)(i0 + r) * a.ldm + (j0 + c) : 0];
      vt[q] = a.M[(j0 + r < n && ic) ? (long)(j0 + r) * a.ldm + (i0 + c) : 0];
    }
    wnext = a.bits[(size_t)(j0 / PT_CHUNK) * np1 + pc];
  };
  fetch(0);
  for (int j0 = 0; j0 < n; j0 += PT_CHUNK) {
    __syncthreads();                         // the previous chunk's operand reads are done
    const bool jc = j0 + c < n, ic = i0 + c < n;
#pragma unroll
    for (int q = 0; q < PT_ROWS / 8; ++q) {
      const int r = r8 + 8 * q;
      As[r * PT_LD + c] = (i0 + r < n && jc) ? va[q] : 0.f;
      At[r * PT_LD + c] = (j0 + r < n && ic) ? vt[q] : 0.f;
    }
    const unsigned w = wnext;                // this lane's labelling on the chunk's 32 partners
    const unsigned live = n - j0 >= PT_CHUNK ? 0xffffffffu : (1u << (n - j0)) - 1u;      // the partners j < n
    __syncthreads();
    if (j0 + PT_CHUNK < n) fetch(j0 + PT_CHUNK);
    f32x16 y1, y0;
#pragma unroll
    for (int r = 0; r < 16; ++r) { y1[r] = 0.f; y0[r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < PT_CHUNK / 2; ++kk) {
      const int k = 2 * kk + half;           // A[i = col][k = half], B[k = half][labelling = col]
      float s = As[col * PT_LD + k] + At[k * PT_LD + col];
      s = (i0 + col == j0 + k) ? 0.f : s;    // the diagonal is never used (a select: a NaN there stays out)
      const float b1 = (w >> k) & 1u ? 1.f : 0.f;
      const float b0 = ((live & ~w) >> k) & 1u ? 1.f : 0.f;
      y1 = __builtin_amdgcn_mfma_f32_32x32x2f32(s, b1, y1, 0, 0, 0);
      y0 = __builtin_amdgcn_mfma_f32_32x32x2f32(s, b0, y0, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool one = (rowmask >> r) & 1u;
      const double d1 = (double)y1[r], d0 = (double)y0[r];
      s11 += one ? d1 : 0.0;
      s01 += one ? d0 : 0.0;
      s00 += one ? 0.0 : d0;
    }
  }
  s00 += __shfl_xor(s00, 32, 64);            // rows 4h + ...: the other half's sum (a + b and b + a have the same bits)
  s11 += __shfl_xor(s11, 32, 64);
  s01 += __shfl_xor(s01, 32, 64);
  if (half == 0 && plive) {
    double* dst = a.part + (size_t)tile * 3 * np1 + p;
    dst[0] = s00; dst[np1] = s11; dst[2 * (size_t)np1] = s01;
  }
}

__global__ __launch_bounds__(256) void perm_stats_kernel(const double* __restrict__ part, int tiles, int np1, double a00, double a01,
                                                         double a11, double* __restrict__ stats) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= np1) return;
  double s00 = 0.0, s11 = 0.0, s01 = 0.0;
  for (int q = 0; q < tiles; ++q) {
    const double* src = part + (size_t)q * 3 * np1 + p;
    s00 += src[0]; s11 += src[np1]; s01 += src[2 * (size_t)np1];
  }
  stats[p] = a00 * (0.5 * s00) + a11 * (0.5 * s11) + a01 * s01;
}

__global__ __launch_bounds__(1024) void perm_count_kernel(const double* __restrict__ stats, int np1, int* __restrict__ count) {
  __shared__ int red[16];
  const double s0 = stats[0];
  int cnt = 0;
  for (int p = 1 + threadIdx.x; p < np1; p += 1024) cnt += stats[p] >= s0 ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < 16; ++w) tot += red[w];
    count[0] = tot;
  }
}

// ---- the Gram matrix of two samples, tiled
struct GramArgs { const float* s1; const float* s2; long ld1, ld2; MmdCfg cfg; float* out; };

__global__ __launch_bounds__(ST_THREADS) void rbf_gram_kernel(GramArgs a) {
  __shared__ float Z[2 * ST_TILE * ST_XS];   // rows 0..63: the tile's rows i, 64..127: its columns j; row stride cfg.zs = d | 1
  __shared__ float nrm[2 * ST_TILE];
  const MmdCfg& c = a.cfg;
  const int n = c.n1 + c.n2, t = threadIdx.x;
  const int i0 = blockIdx.y * ST_TILE, j0 = blockIdx.x * ST_TILE;
  for (int e = t; e < 2 * ST_TILE * c.d; e += ST_THREADS) {
    const int r = e / c.d, k = e - r * c.d;
    const int g = (r < ST_TILE ? i0 + r : j0 + (r - ST_TILE));
    float v = 0.f;
    if (g < n) v = g < c.n1 ? a.s1[(long)g * a.ld1 + k] : a.s2[(long)(g - c.n1) * a.ld2 + k];
    Z[r * c.zs + k] = v;
  }
  __syncthreads();
  if (t < 2 * ST_TILE) {
    float s = 0.f;
    for (int k = 0; k < c.d; ++k) s = fmaf(Z[t * c.zs + k], Z[t * c.zs + k], s);
    nrm[t] = s;
  }
  __syncthreads();
  for (int e = t; e < ST_TILE * ST_TILE; e += ST_THREADS) {
    const int ii = e / ST_TILE, jj = e - ii * ST_TILE;
    if (i0 + ii < n && j0 + jj < n)
      a.out[(size_t)(i0 + ii) * n + (j0 + jj)] = mmd_pair_kernel(c, Z, nrm, ii, ST_TILE + jj, nullptr);
  }
}

// z = [mu_e + eps_e e^lv_e | mu_c + eps_c e^lv_c] of every row of lat with ONE noise pair: sample_z of tail_device.h
__global__ __launch_bounds__(256) void latent_sample_kernel(const float* __restrict__ lat, const float* __restrict__ eps_e,
                                                            const float* __restrict__ eps_c, long total, int D, float* __restrict__ z) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long b = e / (2 * D);
  z[e] = sample_z(lat + b * 4 * D, eps_e, eps_c, D, (int)(e - b * 2 * D));
}

}  // namespace carel

using namespace carel;

void carel::perm_count(const double* stats, int np1, int* count, hipStream_t stream) {
  hipLaunchKernelGGL(perm_count_kernel, dim3(1), dim3(1024), 0, stream, stats, np1, count);
}

static int perm_tiles(int n) { return (n + PT_ROWS - 1) / PT_ROWS; }

extern "C" int64_t carel_mmd_perm_workspace_bytes(int32_t n, int32_t n_permutations) {
  if (n < 4 || n > STAT_MAX_ROWS || n_permutations < 1 || n_permutations > PERM_MAX_P) return 0;
  const int64_t cells = (int64_t)perm_tiles(n) * ((int64_t)n_permutations + 1);      // (row tile, labelling): three doubles and one label word
  return 8 * (3 * cells + (cells + 1) / 2);
}

extern "C" int carel_mmd_perm_test(const carel_mmd_perm_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "carel_mmd_perm_test";
  if (!a || !a->matrix || !a->labels || !a->stats || !a->count || !a->workspace) return set_error(CAREL_ERR_ARG, "%s: null pointer", who);
  if (a->n1 < 2 || a->n2 < 2) return set_error(CAREL_ERR_SHAPE, "%s: n1,n2 must be >= 2", who);
  const long n = (long)a->n1 + a->n2;
  if (n > STAT_MAX_ROWS) return set_error(CAREL_ERR_SHAPE, "%s: n1 + n2 must be <= %d (got %ld)", who, STAT_MAX_ROWS, n);
  if (a->n_permutations < 1 || a->n_permutations > PERM_MAX_P)
    return set_error(CAREL_ERR_SHAPE, "%s: n_permutations must be in 1..%d (got %d)", who, PERM_MAX_P, a->n_permutations);
  if (a->ldm < n) return set_error(CAREL_ERR_ARG, "%s: row stride %lld below n = %ld", who, (long long)a->ldm, n);
  const int64_t need = carel_mmd_perm_workspace_bytes((int32_t)n, a->n_permutations);
  if (int rc = check_workspace(who, a->workspace, 1, a->workspace_bytes, need)) return rc;      // (1: this entry demands no alignment)
  PermArgs k;
  k.M = (const float*)a->matrix; k.ldm = a->ldm; k.labels = (const unsigned char*)a->labels;
  k.n = (int)n; k.np1 = a->n_permutations + 1; k.part = (double*)a->workspace;
  const int tiles = perm_tiles(k.n);
  k.bits = (unsigned*)(k.part + (size_t)tiles * 3 * k.np1);
  hipLaunchKernelGGL(perm_pack_kernel, dim3((unsigned)(((long)tiles * k.np1 + 255) / 256)), dim3(256), 0, stream, k, tiles);
  hipLaunchKernelGGL(perm_tile_kernel, dim3(tiles, (k.np1 + PT_LABS - 1) / PT_LABS), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(perm_stats_kernel, dim3((k.np1 + 255) / 256), dim3(256), 0, stream, (const double*)k.part, tiles, k.np1, a->a00, a->a01,
                     a->a11, (double*)a->stats);
  perm_count((const double*)a->stats, k.np1, (int*)a->count, stream);
  return check_launch("carel_mmd_perm_test");
}

extern "C" int carel_rbf_gram(const carel_mmd_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "carel_rbf_gram";
  if (!a || !a->s1 || !a->s2 || !a->kernels_out) return set_error(CAREL_ERR_ARG, "%s: null pointer", who);
  if (a->n1 < 1 || a->n2 < 1) return set_error(CAREL_ERR_SHAPE, "%s: empty sample", who);
  const long n = (long)a->n1 + a->n2;
  if (n > STAT_MAX_ROWS) return set_error(CAREL_ERR_SHAPE, "%s: n1 + n2 must be <= %d (got %ld)", who, STAT_MAX_ROWS, n);
  if (a->d < 1 || a->d > STAT_MAX_D) return set_error(CAREL_ERR_SHAPE, "%s: d must be in 1..%d (got %d)", who, STAT_MAX_D, a->d);
  if (a->n_alphas < 1 || a->n_alphas > 8) return set_error(CAREL_ERR_ARG, "%s: n_alphas must be in 1..8", who);
  if (a->ld1 < a->d || a->ld2 < a->d) return set_error(CAREL_ERR_ARG, "%s: row stride below d", who);
  GramArgs k;
  k.s1 = (const float*)a->s1; k.s2 = (const float*)a->s2; k.ld1 = a->ld1; k.ld2 = a->ld2;
  fill_mmd_cfg(&k.cfg, a, a->d | 1);
  k.out = (float*)a->kernels_out;
  const int tiles = (int)((n + ST_TILE - 1) / ST_TILE);
  hipLaunchKernelGGL(rbf_gram_kernel, dim3(tiles, tiles), dim3(ST_THREADS), 0, stream, k);
  return check_launch("rbf_gram_kernel");
}

extern "C" int carel_sample_latents(const void* lat, const void* eps_e, const void* eps_c, int32_t n, int32_t ec_dim, void* z, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "carel_sample_latents";
  if (!lat || !eps_e || !eps_c || !z) return set_error(CAREL_ERR_ARG, "%s: null pointer", who);
  if (n < 1) return set_error(CAREL_ERR_SHAPE, "%s: n must be >= 1", who);
  if (ec_dim < 1 || ec_dim > 32) return set_error(CAREL_ERR_SHAPE, "%s: ec_dim must be in 1..32", who);
  const long total = (long)n * 2 * ec_dim;
  hipLaunchKernelGGL(latent_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const float*)lat, (const float*)eps_e,
                     (const float*)eps_c, total, ec_dim, (float*)z);
  return check_launch("latent_sample_kernel");
}
