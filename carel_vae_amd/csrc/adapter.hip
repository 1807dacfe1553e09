// Sentence adapters of drl_classifier_ec_mmd_final_mul_emnlp.py (:162-256 classes, :273-291 construction, :334-354 forward):
// a fixed query per branch attends over every position of the last hidden state H [B, S, 768], normalised by softmax (raw
// nn.MultiheadAttention), sparsemax or entmax-1.5.  The key projection is reassociated into one vector per query,
// u = W_k^T q / sqrt(d) (the normalisers are translation-invariant, so the key bias drops out), and scores are H . u.
//
//   forward : rowdot (scores of every row against the 2G u vectors)  ->  normalise (one wave per score row)  ->  combine (the p-weighted
//             row sums, one workgroup per sample and 64 columns)  [-> raw: value projection and out_proj GEMVs]
//   backward: [raw: out_proj^T and value^T GEMVs]  ->  rowdot (dp = H . dctx)  ->  dzdh (normaliser backward, dH rows)
//   weights : (opt-in, after the backward)  wgrad_dz (the normaliser backward again, stored)  ->  combine (du partials per sample, the one
//             pass over H)  ->  wgrad_dusum (samples in ascending order)  ->  gemv (dqv = W_k du)  ->  wgrad_outer (every rank-1 / rank-B product)
// Every sum has a fixed order; no atomics.
#include "carel_hip_internal.h"

namespace carel {

constexpr int AD = 768;              // hidden width
constexpr int AD4 = AD / 4;
constexpr int RD_ROWS = 16;          // rowdot: rows per workgroup (four waves x four rows)
constexpr int CB_COLS = 64;          // combine: columns per workgroup
constexpr int DZ_ROWS = 8;           // dzdh: rows per workgroup

// LDS written by some lanes of a wave, then read by others of the same wave (a wave's LDS operations complete in order)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave normalises one row z[0..S) (S <= 128, LDS) into p[0..S) (LDS); sh / srt: this wave's LDS scratch [128] each.
// Lane l owns positions l and l + 64.  The sort-based forms are those of the entmax / sparsemax packages:
//   sparsemax: z -= max z; sorted descending zs; k* = max{k : 1 + k zs_k > sum_{j<=k} zs_j}; tau = (sum_{those k} zs_k - 1) / k*
//   entmax15 : x = (z - max z) / 2; for each k: mean_k, ss_k = sum_{j<=k} (xs_j - mean_k)^2, tau_k = mean_k - sqrt(max((1 - ss_k)/k, 0));
//              support = #{k : tau_k <= xs_k}; p = max(x - tau_support, 0)^2
// Sorting is by rank (count of larger values, ties broken by index): exact, and the sorted values equal torch.sort's.
__device__ void wave_normalise(int mode, const float* z, float* p, float* sh, float* srt, int S, int lane) {
  const bool v0 = lane < S, v1 = lane + 64 < S;
  float z0 = v0 ? z[lane] : -INFINITY, z1 = v1 ? z[lane + 64] : -INFINITY;
  const float m = wave_max(fmaxf(z0, z1));
  if (mode == 0) {
    const float e0 = v0 ? expf(z0 - m) : 0.f, e1 = v1 ? expf(z1 - m) : 0.f;
    const float inv = 1.0f / wave_sum(e0 + e1);
    if (v0) p[lane] = e0 * inv;
    if (v1) p[lane + 64] = e1 * inv;
    return;
  }
  const float x0 = v0 ? (mode == 2 ? (z0 - m) / 2 : z0 - m) : 0.f;
  const float x1 = v1 ? (mode == 2 ? (z1 - m) / 2 : z1 - m) : 0.f;
  if (v0) sh[lane] = x0;
  if (v1) sh[lane + 64] = x1;
  wave_lds_sync();
  int r0 = 0, r1 = 0;
  for (int j = 0; j < S; ++j) {
    const float y = sh[j];
    r0 += (y > x0) || (y == x0 && j < lane);
    r1 += (y > x1) || (y == x1 && j < lane + 64);
  }
  if (v0) srt[r0] = x0;
  if (v1) srt[r1] = x1;
  wave_lds_sync();
  // lane owns sorted positions k0 = lane, k1 = lane + 64 (0-based); prefix sums by a fixed sequential loop
  const int k0 = lane, k1 = lane + 64;
  float c0 = 0.f, c1 = 0.f;
  for (int j = 0; j < S; ++j) {
    const float y = srt[j];
    if (j <= k0) c0 += y;
    if (j <= k1) c1 += y;
  }
  const float s0 = v0 ? srt[k0] : 0.f, s1 = v1 ? srt[k1] : 0.f;
  float tau;
  if (mode == 1) {
    const bool g0 = v0 && (1.0f + (float)(k0 + 1) * s0 > c0), g1 = v1 && (1.0f + (float)(k1 + 1) * s1 > c1);
    const float kstar = wave_max(fmaxf(g0 ? (float)(k0 + 1) : 0.f, g1 ? (float)(k1 + 1) : 0.f));
    const float sgt = wave_sum((g0 ? s0 : 0.f) + (g1 ? s1 : 0.f));
    tau = (sgt - 1.0f) / kstar;
    if (v0) p[lane] = fmaxf(x0 - tau, 0.f);
    if (v1) p[lane + 64] = fmaxf(x1 - tau, 0.f);
    return;
  }
  const float mean0 = c0 / (float)(k0 + 1), mean1 = c1 / (float)(k1 + 1);
  float ss0 = 0.f, ss1 = 0.f;
  for (int j = 0; j < S; ++j) {
    const float y = srt[j];
    const float d0 = y - mean0, d1 = y - mean1;
    if (j <= k0) ss0 = fmaf(d0, d0, ss0);
    if (j <= k1) ss1 = fmaf(d1, d1, ss1);
  }
  const float t0 = mean0 - sqrtf(fmaxf((1.0f - ss0) / (float)(k0 + 1), 0.f));
  const float t1 = mean1 - sqrtf(fmaxf((1.0f - ss1) / (float)(k1 + 1), 0.f));
  const int support = (int)wave_sum((v0 && t0 <= s0 ? 1.f : 0.f) + (v1 && t1 <= s1 ? 1.f : 0.f));   // >= 1: tau_1 = xs_1 - 1
  const int ks = support - 1;
  const float ta = __shfl(t0, ks & 63, 64), tb = __shfl(t1, ks & 63, 64);
  tau = ks < 64 ? ta : tb;
  if (v0) { const float d = fmaxf(x0 - tau, 0.f); p[lane] = d * d; }
  if (v1) { const float d = fmaxf(x1 - tau, 0.f); p[lane + 64] = d * d; }
}

// Softmax backward of one row, two values per lane (p = 0, dp = 0 beyond S):  dz = p ((dp - c) - sum p (dp - c)),  c = dp at the largest p
// (the lowest index on a tie).  For sum p = 1 that is p (dp - sum p dp); in float32 the p of a nearly one-hot row miss sum p = 1 by a
// rounding, and the plain form loses the dominant token's dz -- a difference of nearly equal numbers -- to it.  With the shift the
// dominant term of the sum is an exact zero and every other term is small.
__device__ __forceinline__ void softmax_backward(float p0, float p1, float g0, float g1, int lane, float& r0, float& r1) {
  const float pm = wave_max(fmaxf(p0, p1));
  const float at = p0 == pm ? (float)lane : (p1 == pm ? (float)(lane + 64) : 128.f);
  const int idx = (int)-wave_max(-at);
  const float ca = __shfl(g0, idx & 63, 64), cb = __shfl(g1, idx & 63, 64);
  const float c = idx < 64 ? ca : cb;
  const float h0 = g0 - c, h1 = g1 - c;
  const float sp = wave_sum(p0 * h0 + p1 * h1);
  r0 = p0 * (h0 - sp); r1 = p1 * (h1 - sp);
}

// out[k][b][s] = x[b*S + s] . vec_k(b),  k = a*G + g,  vec_k(b) = vec + a*v_as + b*v_bs + g*768.  Grid (S / 16, B).
template <int NV>
__global__ __launch_bounds__(256) void adapter_rowdot_kernel(const float* __restrict__ x, int S, int B, const float* __restrict__ vec,
                                                             long v_as, long v_bs, int G, float* __restrict__ out) {
  __shared__ float4 vs[NV * AD4];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < NV * AD4; i += 256) {
    const int k = i / AD4, c = i - k * AD4, a = k / G, g = k - a * G;
    vs[i] = *(const float4*)(vec + a * v_as + b * v_bs + (long)g * AD + c * 4);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int s0 = blockIdx.x * RD_ROWS + w * 4;
  float4 xv[4][3];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float* row = x + ((long)b * S + s0 + r) * AD;
#pragma unroll
    for (int i = 0; i < 3; ++i) xv[r][i] = *(const float4*)(row + (i * 64 + lane) * 4);
  }
  float part[4][NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float4 uv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) uv[i] = vs[k * AD4 + i * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i) t += (xv[r][i].x * uv[i].x + xv[r][i].y * uv[i].y) + (xv[r][i].z * uv[i].z + xv[r][i].w * uv[i].w);
      part[r][k] = t;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int k = 0; k < NV; ++k) part[r][k] += __shfl_xor(part[r][k], off, 64);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[((long)k * B + b) * S + s0 + r] = part[r][k];
    }
  }
}

// p[r] = normaliser(sc[r]) for the `rows` score rows of S values (r = k*B + b): one wave per row, once per row.  Grid ceil(rows / 4).
__global__ __launch_bounds__(256) void adapter_normalise_kernel(int rows, int S, int mode, const float* __restrict__ sc, float* __restrict__ p) {
  __shared__ float scratch[4][2][128];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = blockIdx.x * 4 + w;
  if (r >= rows) return;                     // wave-uniform
  wave_normalise(mode, sc + (long)r * S, p + (long)r * S, scratch[w][0], scratch[w][1], S, lane);
}

// ctx_k[b][cols] = sum_s p[k][b][s] x[b*S + s][cols] for this workgroup's 64 columns.  ctx_k = out + a*o_as + b*o_bs + g*768.
// Grid (768 / 64, B), 256 threads: 16 row groups x 16 float4 columns.
template <int NV>
__global__ __launch_bounds__(256) void adapter_combine_kernel(const float* __restrict__ x, int S, int B, int G, const float* __restrict__ p,
                                                              float* __restrict__ out, long o_as, long o_bs) {
  __shared__ float ps[NV][128];
  __shared__ float4 red[4][NV][16];
  const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int i = t; i < NV * S; i += 256) {
    const int k = i / S, s = i - k * S;
    ps[k][s] = p[((long)k * B + b) * S + s];
  }
  __syncthreads();
  const int c4 = t & 15, rg = t >> 4;
  const int col = blockIdx.x * CB_COLS + c4 * 4;
  float4 acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = float4{0.f, 0.f, 0.f, 0.f};
  for (int s = rg; s < S; s += 16) {
    const float4 h = *(const float4*)(x + ((long)b * S + s) * AD + col);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const float pk = ps[k][s];
      acc[k].x = fmaf(pk, h.x, acc[k].x); acc[k].y = fmaf(pk, h.y, acc[k].y);
      acc[k].z = fmaf(pk, h.z, acc[k].z); acc[k].w = fmaf(pk, h.w, acc[k].w);
    }
  }
#pragma unroll
  for (int off = 16; off < 64; off <<= 1) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      acc[k].x += __shfl_xor(acc[k].x, off, 64); acc[k].y += __shfl_xor(acc[k].y, off, 64);
      acc[k].z += __shfl_xor(acc[k].z, off, 64); acc[k].w += __shfl_xor(acc[k].w, off, 64);
    }
  }
  if (lane < 16) {
#pragma unroll
    for (int k = 0; k < NV; ++k) red[w][k][lane] = acc[k];
  }
  __syncthreads();
  for (int i = t; i < NV * 16; i += 256) {
    const int k = i >> 4, c = i & 15, a = k / G, g = k - a * G;
    float4 v = red[0][k][c];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) { const float4 q = red[ww][k][c]; v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
    *(float4*)(out + a * o_as + (long)b * o_bs + (long)g * AD + blockIdx.x * CB_COLS + c * 4) = v;
  }
}

// Normaliser backward for sample b (every workgroup of the sample re-derives it) and the dH rows of this workgroup:
//   dH[b*S + s] = sum_k p[k][b][s] dctx_k(b) + dz[k][b][s] u_k,  dctx_k(b) = dctx + a*d_as + b*d_bs + g*768,  u_k = u + k*768.
// Filler samples (b >= B) get zero rows.  Grid (S / 8, Bp), 192 threads (one float4 column each).
template <int NV>
__global__ __launch_bounds__(192) void adapter_dzdh_kernel(int S, int B, int G, int mode, const float* __restrict__ p, const float* __restrict__ dp,
                                                           const float* __restrict__ dctx, long d_as, long d_bs, const float* __restrict__ u,
                                                           float* __restrict__ dx) {
  __shared__ float pl[NV][128];
  __shared__ float dz[NV][128];
  const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int s0 = blockIdx.x * DZ_ROWS;
  if (b >= B) {
#pragma unroll
    for (int r = 0; r < DZ_ROWS; ++r) *(float4*)(dx + ((long)b * S + s0 + r) * AD + t * 4) = float4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  for (int i = t; i < NV * S; i += 192) {
    const int k = i / S, s = i - k * S;
    pl[k][s] = p[((long)k * B + b) * S + s];
    dz[k][s] = dp[((long)k * B + b) * S + s];
  }
  __syncthreads();
  for (int k = w; k < NV; k += 3) {
    const bool v0 = lane < S, v1 = lane + 64 < S;
    const float p0 = v0 ? pl[k][lane] : 0.f, p1 = v1 ? pl[k][lane + 64] : 0.f;
    const float g0 = v0 ? dz[k][lane] : 0.f, g1 = v1 ? dz[k][lane + 64] : 0.f;
    float r0, r1;
    if (mode == 0) {
      softmax_backward(p0, p1, g0, g1, lane, r0, r1);
    } else if (mode == 1) {
      const float n = wave_sum((p0 > 0.f ? 1.f : 0.f) + (p1 > 0.f ? 1.f : 0.f));
      const float mean = wave_sum((p0 > 0.f ? g0 : 0.f) + (p1 > 0.f ? g1 : 0.f)) / n;
      r0 = p0 > 0.f ? g0 - mean : 0.f; r1 = p1 > 0.f ? g1 - mean : 0.f;
    } else {
      const float q0 = sqrtf(p0), q1 = sqrtf(p1);
      const float d0 = g0 * q0, d1 = g1 * q1;
      const float qq = wave_sum(d0 + d1) / wave_sum(q0 + q1);
      r0 = d0 - qq * q0; r1 = d1 - qq * q1;
    }
    if (v0) dz[k][lane] = r0;
    if (v1) dz[k][lane + 64] = r1;
  }
  __syncthreads();
  float4 acc[DZ_ROWS];
#pragma unroll
  for (int r = 0; r < DZ_ROWS; ++r) acc[r] = float4{0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < NV; ++k) {
    const int a = k / G, g = k - a * G;
    const float4 d4 = *(const float4*)(dctx + a * d_as + (long)b * d_bs + (long)g * AD + t * 4);
    const float4 u4 = *(const float4*)(u + (long)k * AD + t * 4);
#pragma unroll
    for (int r = 0; r < DZ_ROWS; ++r) {
      const float pk = pl[k][s0 + r], zk = dz[k][s0 + r];
      acc[r].x = fmaf(zk, u4.x, fmaf(pk, d4.x, acc[r].x)); acc[r].y = fmaf(zk, u4.y, fmaf(pk, d4.y, acc[r].y));
      acc[r].z = fmaf(zk, u4.z, fmaf(pk, d4.z, acc[r].z)); acc[r].w = fmaf(zk, u4.w, fmaf(pk, d4.w, acc[r].w));
    }
  }
#pragma unroll
  for (int r = 0; r < DZ_ROWS; ++r) *(float4*)(dx + ((long)b * S + s0 + r) * AD + t * 4) = acc[r];
}

// out[a][b][n] = sum_k W_a[n][k] in[a][b][n / seg][k] + bias_a[n]   (one wave per (n, a); samples four at a time).
// in = in_base + a*i_as + b*i_bs + (n / seg)*768.
struct AdPtr2 { const float* w[2]; const float* b[2]; };
__global__ __launch_bounds__(256) void adapter_gemv_kernel(AdPtr2 W, const float* __restrict__ in, long i_as, long i_bs, int seg, int B,
                                                           float* __restrict__ out, long o_as, long o_bs) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), a = blockIdx.y;
  const float* wr = W.w[a] + (long)n * AD;
  const float bias = W.b[a] ? W.b[a][n] : 0.f;
  float4 wv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) wv[i] = *(const float4*)(wr + (i * 64 + lane) * 4);
  const float* ib = in + a * i_as + (long)(n / seg) * AD;
  for (int b = 0; b < B; b += 4) {
    float s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float* xr = ib + (long)min(b + q, B - 1) * i_bs;
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float4 xv = *(const float4*)(xr + (i * 64 + lane) * 4);
        t += (xv.x * wv[i].x + xv.y * wv[i].y) + (xv.z * wv[i].z + xv.w * wv[i].w);
      }
      s[q] = t;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] += __shfl_xor(s[q], off, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) if (b + q < B) out[a * o_as + (long)(b + q) * o_bs + n] = s[q] + bias;
    }
  }
}

// Transposed form  out[a][b][g][k] = scale * sum_{n in [g*seg, (g+1)*seg)} W_a[n][k] in[a][b][n]  in two launches that fill the chip:
// gemvT_part: the 768 rows n in 24 chunks of 32, part[c][a][b][k] (one thread per k, eight samples per workgroup),
//             grid (768 / 256, 24, 2 * ceil(B / 8));  in = in_base + a*i_as + b*i_bs
// gemvT_sum : the chunks of each head g = n / seg added in ascending order (seg is a multiple of 32 for every G | 768, G <= 12).
constexpr int GT_B = 8;
constexpr int GT_N = 32;
constexpr int GT_C = AD / GT_N;
__global__ __launch_bounds__(256) void adapter_gemvT_part_kernel(AdPtr2 W, const float* __restrict__ in, long i_as, long i_bs, int B,
                                                                 float* __restrict__ part) {
  const int k = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  const int nbc = (B + GT_B - 1) / GT_B, a = blockIdx.z / nbc, b0 = (blockIdx.z - a * nbc) * GT_B;
  const float* wa = W.w[a];
  const float* ia = in + a * i_as;
  float acc[GT_B];
#pragma unroll
  for (int q = 0; q < GT_B; ++q) acc[q] = 0.f;
#pragma unroll 8
  for (int n = c * GT_N; n < (c + 1) * GT_N; ++n) {
    const float wk = wa[(long)n * AD + k];
#pragma unroll
    for (int q = 0; q < GT_B; ++q) acc[q] = fmaf(wk, ia[(long)min(b0 + q, B - 1) * i_bs + n], acc[q]);
  }
#pragma unroll
  for (int q = 0; q < GT_B; ++q)
    if (b0 + q < B) part[(((long)c * 2 + a) * B + b0 + q) * AD + k] = acc[q];
}
__global__ __launch_bounds__(256) void adapter_gemvT_sum_kernel(const float* __restrict__ part, int B, int G, float scale,
                                                                float* __restrict__ out, long o_as, long o_bs) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;       // (a, b, g, k)
  if (i >= 2L * B * G * AD) return;
  const int k = (int)(i % AD), g = (int)((i / AD) % G), b = (int)((i / ((long)AD * G)) % B), a = (int)(i / ((long)AD * G * B));
  const int cpg = GT_C / G;
  float v = 0.f;
  for (int c = g * cpg; c < (g + 1) * cpg; ++c) v += part[(((long)c * 2 + a) * B + b) * AD + k];
  out[a * o_as + (long)b * o_bs + (long)g * AD + k] = v * scale;
}
static void gemvT(AdPtr2 W, const float* in, long i_as, long i_bs, int B, int G, float scale, float* out, long o_as, long o_bs, float* part,
                  hipStream_t stream) {
  const int nbc = (B + GT_B - 1) / GT_B;
  hipLaunchKernelGGL(adapter_gemvT_part_kernel, dim3(AD / 256, GT_C, 2 * nbc), dim3(256), 0, stream, W, in, i_as, i_bs, B, part);
  hipLaunchKernelGGL(adapter_gemvT_sum_kernel, dim3((unsigned)((2L * B * G * AD + 255) / 256)), dim3(256), 0, stream, (const float*)part, B, G,
                     scale, out, o_as, o_bs);
}

// ---- weight gradients (carel_adapter_backward_weights; opt-in, nothing above calls these) ----
// dz[r][0..S) = normaliser backward of score row r = k*B + b from p[r] and dp[r]: the expressions of adapter_dzdh_kernel, so that the
// weight gradients and dH differentiate the same function.  One wave per row.  Grid ceil(rows / 4).
__global__ __launch_bounds__(256) void adapter_wgrad_dz_kernel(int rows, int S, int mode, const float* __restrict__ p, const float* __restrict__ dp,
                                                               float* __restrict__ dz) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                     // wave-uniform
  const float* pr = p + (long)r * S;
  const float* gr = dp + (long)r * S;
  const bool v0 = lane < S, v1 = lane + 64 < S;
  const float p0 = v0 ? pr[lane] : 0.f, p1 = v1 ? pr[lane + 64] : 0.f;
  const float g0 = v0 ? gr[lane] : 0.f, g1 = v1 ? gr[lane + 64] : 0.f;
  float r0, r1;
  if (mode == 0) {
    softmax_backward(p0, p1, g0, g1, lane, r0, r1);
  } else if (mode == 1) {
    const float n = wave_sum((p0 > 0.f ? 1.f : 0.f) + (p1 > 0.f ? 1.f : 0.f));
    const float mean = wave_sum((p0 > 0.f ? g0 : 0.f) + (p1 > 0.f ? g1 : 0.f)) / n;
    r0 = p0 > 0.f ? g0 - mean : 0.f; r1 = p1 > 0.f ? g1 - mean : 0.f;
  } else {
    const float q0 = sqrtf(p0), q1 = sqrtf(p1);
    const float d0 = g0 * q0, d1 = g1 * q1;
    const float qq = wave_sum(d0 + d1) / wave_sum(q0 + q1);
    r0 = d0 - qq * q0; r1 = d1 - qq * q1;
  }
  if (v0) dz[(long)r * S + lane] = r0;
  if (v1) dz[(long)r * S + lane + 64] = r1;
}

// du[a][g][:] = scale * sum_b part[a][b][g][:], the samples in ascending order.  Grid ceil(2 G 768 / 256).
__global__ __launch_bounds__(256) void adapter_wgrad_dusum_kernel(const float* __restrict__ part, int B, int G, float scale, float* __restrict__ du) {
  const int i = blockIdx.x * 256 + threadIdx.x, per = G * AD;
  if (i >= 2 * per) return;
  const int a = i / per;
  const float* src = part + (long)a * B * per + (i - a * per);
  float v = 0.f;
#pragma unroll 8
  for (int b = 0; b < B; ++b) v += src[(long)b * per];
  du[i] = v * scale;
}

// Rank-nb updates, one job per blockIdx.z:
//   dW_a[n][:] (+)= sum_{b < nb} L_a[b*l_bs + n] * R_a[b*r_bs + (n / seg)*768 + :]      db_a[n] (+)= sum_{b < nb} L_a[b*l_bs + n]
// (bias 1: that sum; 2: zeros, the key bias; db NULL: none), b ascending; (+)= adds when accumulate, else overwrites.
// Grid (768 / 8, 2, jobs), 192 threads (one float4 column each); the 8 rows of a workgroup share a head (seg is a multiple of 8).
constexpr int OW_ROWS = 8;
struct AdOuterJob { const float* L[2]; const float* R[2]; float* dW[2]; float* db[2]; long l_bs, r_bs; int nb, seg, bias; };
struct AdOuterJobs { AdOuterJob j[4]; };
__global__ __launch_bounds__(192) void adapter_wgrad_outer_kernel(AdOuterJobs J, int accumulate) {
  const AdOuterJob& j = J.j[blockIdx.z];
  const int a = blockIdx.y, n0 = blockIdx.x * OW_ROWS, t = threadIdx.x;
  const float* L = j.L[a] + n0;
  const float* R = j.R[a] + (long)(n0 / j.seg) * AD + t * 4;
  float4 acc[OW_ROWS];
#pragma unroll
  for (int r = 0; r < OW_ROWS; ++r) acc[r] = float4{0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < j.nb; ++b) {
    const float4 r4 = *(const float4*)(R + b * j.r_bs);
#pragma unroll
    for (int r = 0; r < OW_ROWS; ++r) {
      const float l = L[b * j.l_bs + r];
      acc[r].x = fmaf(l, r4.x, acc[r].x); acc[r].y = fmaf(l, r4.y, acc[r].y);
      acc[r].z = fmaf(l, r4.z, acc[r].z); acc[r].w = fmaf(l, r4.w, acc[r].w);
    }
  }
  float* dst = j.dW[a] + (long)n0 * AD + t * 4;
#pragma unroll
  for (int r = 0; r < OW_ROWS; ++r) {
    float4 v = acc[r];
    if (accumulate) { const float4 o = *(const float4*)(dst + (long)r * AD); v.x = o.x + v.x; v.y = o.y + v.y; v.z = o.z + v.z; v.w = o.w + v.w; }
    *(float4*)(dst + (long)r * AD) = v;
  }
  if (j.db[a] && t < OW_ROWS) {
    float s = 0.f;
    if (j.bias == 1)
      for (int b = 0; b < j.nb; ++b) s += L[b * j.l_bs + t];
    float* d = j.db[a] + n0 + t;
    *d = accumulate ? *d + s : s;
  }
}

struct AdWork { float* qv; float* sc; float* p; float* ctx; float* vcat; float* dvcat; float* dctx; float* part; size_t total; };
static size_t ad_align(size_t n) { return (n + 63) & ~(size_t)63; }
static AdWork ad_carve(float* base, int B, int S, int G) {
  AdWork w; size_t o = 0;
  auto take = [&](size_t n) { float* q = base ? base + o : nullptr; o += ad_align(n); return q; };
  const size_t nv = 2 * (size_t)G;
  w.qv = take(2 * AD); w.sc = take(nv * B * S); w.p = take(nv * B * S);
  w.ctx = take(nv * B * AD); w.vcat = take(2 * (size_t)B * AD); w.dvcat = take(2 * (size_t)B * AD); w.dctx = take(nv * B * AD);
  w.part = take((size_t)GT_C * 2 * (B > 1 ? B : 1) * AD);
  w.total = o;
  return w;
}
// carel_adapter_backward_weights' own scratch: dz [2G][B][S <= 128], per-sample du partials [2][B][G][768], du [2][G][768], dqv [2][768]
struct AdWgWork { float* dz; float* part; float* du; float* dqv; size_t total; };
static AdWgWork adwg_carve(float* base, int B, int G) {
  AdWgWork w; size_t o = 0;
  auto take = [&](size_t n) { float* q = base ? base + o : nullptr; o += ad_align(n); return q; };
  const size_t nv = 2 * (size_t)G;
  w.dz = take(nv * B * 128); w.part = take(nv * B * AD); w.du = take(nv * AD); w.dqv = take(2 * AD);
  w.total = o;
  return w;
}

static int ad_check(const carel_adapter_args* a, const char* who) {
  if (!a) return set_error(CAREL_ERR_ARG, "%s: null args", who);
  if (a->mode < 0 || a->mode > 2) return set_error(CAREL_ERR_ARG, "%s: mode must be 0 (raw), 1 (sparsemax) or 2 (entmax15)", who);
  const int G = a->heads;
  if (G < 1 || G > 12 || AD % G) return set_error(CAREL_ERR_SHAPE, "%s: heads must divide 768 and be <= 12 (got %d)", who, G);
  if (a->mode != 0 && G != 1) return set_error(CAREL_ERR_SHAPE, "%s: sparsemax / entmax15 adapters use one query vector (heads = 1)", who);
  if (a->batch < 1 || a->batch_padded < a->batch) return set_error(CAREL_ERR_SHAPE, "%s: need 1 <= batch <= batch_padded", who);
  if (a->seq_len < 32 || a->seq_len > 128 || a->seq_len % 32) return set_error(CAREL_ERR_SHAPE, "%s: seq_len must be 32, 64, 96 or 128", who);
  if (!a->u || !a->work) return set_error(CAREL_ERR_ARG, "%s: null u / work", who);
  // the sample index is a grid y coordinate (rowdot, combine: batch; dzdh: batch_padded)
  if (a->batch_padded > 65535) return set_error(CAREL_ERR_SHAPE, "%s: batch_padded must be <= 65535", who);
  // every kernel moves these as float4 (NULL where a call does not use one: the entry points check that)
  const void* vec[] = {a->u, a->work, a->x_f32, a->out_f32, a->d_out_f32, a->dx_f32, a->query[0], a->query[1], a->q_w[0], a->q_w[1],
                       a->k_w[0], a->k_w[1], a->v_w[0], a->v_w[1], a->o_w[0], a->o_w[1]};
  for (const void* q : vec)
    if ((uintptr_t)q & 15) return set_error(CAREL_ERR_ARG, "%s: u, work, x, out, d_out, dx, query and the weights must be 16-byte aligned", who);
  return CAREL_OK;
}

#define AD_NV_SWITCH(NVV, CALL)                                                                                     \
  switch (NVV) {                                                                                                    \
    case 2: { constexpr int NV = 2; CALL; } break;                                                                  \
    case 4: { constexpr int NV = 4; CALL; } break;                                                                  \
    case 6: { constexpr int NV = 6; CALL; } break;                                                                  \
    case 8: { constexpr int NV = 8; CALL; } break;                                                                  \
    case 12: { constexpr int NV = 12; CALL; } break;                                                                \
    case 16: { constexpr int NV = 16; CALL; } break;                                                                \
    case 24: { constexpr int NV = 24; CALL; } break;                                                                \
    default: return set_error(CAREL_ERR_SHAPE, "adapter: unsupported head count");                                  \
  }

}  // namespace carel

using namespace carel;

extern "C" int64_t carel_adapter_workspace_floats(int32_t batch, int32_t seq_len, int32_t heads) {
  if (batch < 1 || seq_len < 1 || heads < 1) return 0;
  return (int64_t)ad_carve(nullptr, batch, seq_len, heads).total;
}

extern "C" int carel_adapter_build_u(const carel_adapter_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = ad_check(a, "carel_adapter_build_u");
  if (rc) return rc;
  for (int i = 0; i < 2; ++i)
    if (!a->query[i] || !a->q_w[i] || !a->q_b[i] || !a->k_w[i]) return set_error(CAREL_ERR_ARG, "carel_adapter_build_u: null query / weight");
  const int G = a->heads;
  AdWork w = ad_carve((float*)a->work, a->batch, a->seq_len, G);
  // q = W_q e + b_q: one "sample" per adapter (the query vectors are separate tensors: two launches of one sample each)
  for (int i = 0; i < 2; ++i) {
    AdPtr2 W = {{(const float*)a->q_w[i], (const float*)a->q_w[i]}, {(const float*)a->q_b[i], (const float*)a->q_b[i]}};
    hipLaunchKernelGGL(adapter_gemv_kernel, dim3(AD / 4, 1), dim3(256), 0, stream, W, (const float*)a->query[i], 0L, 0L, AD, 1,
                       w.qv + i * AD, 0L, 0L);
  }
  // u[a][g] = W_k,g^T q_g / sqrt(768 / G)
  AdPtr2 K = {{(const float*)a->k_w[0], (const float*)a->k_w[1]}, {nullptr, nullptr}};
  const int dh = AD / G;
  gemvT(K, (const float*)w.qv, (long)AD, 0L, 1, G, 1.0f / sqrtf((float)dh), (float*)a->u, (long)G * AD, 0L, w.part, stream);
  return check_launch("carel_adapter_build_u");
}

extern "C" int carel_adapter_forward(const carel_adapter_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = ad_check(a, "carel_adapter_forward");
  if (rc) return rc;
  if (!a->x_f32 || !a->out_f32) return set_error(CAREL_ERR_ARG, "carel_adapter_forward: null x / out");
  if (a->mode == 0)
    for (int i = 0; i < 2; ++i)
      if (!a->v_w[i] || !a->v_b[i] || !a->o_w[i] || !a->o_b[i]) return set_error(CAREL_ERR_ARG, "carel_adapter_forward: raw mode needs v_* / o_*");
  const int B = a->batch, S = a->seq_len, G = a->heads, nv = 2 * G;
  AdWork w = ad_carve((float*)a->work, B, S, G);
  const float* x = (const float*)a->x_f32;
  AD_NV_SWITCH(nv, hipLaunchKernelGGL(adapter_rowdot_kernel<NV>, dim3(S / RD_ROWS, B), dim3(256), 0, stream, x, S, B, (const float*)a->u,
                                      (long)G * AD, 0L, G, w.sc));
  // sparse modes: the weighted sums are the adapter outputs; raw: per-head contexts [2][B][G][768]
  float* ctx = a->mode == 0 ? w.ctx : (float*)a->out_f32;
  const long c_as = (long)B * G * AD, c_bs = (long)G * AD;
  hipLaunchKernelGGL(adapter_normalise_kernel, dim3((nv * B + 3) / 4), dim3(256), 0, stream, nv * B, S, a->mode, (const float*)w.sc, w.p);
  AD_NV_SWITCH(nv, hipLaunchKernelGGL(adapter_combine_kernel<NV>, dim3(AD / CB_COLS, B), dim3(256), 0, stream, x, S, B, G, (const float*)w.p,
                                      ctx, c_as, c_bs));
  if (a->mode == 0) {
    AdPtr2 V = {{(const float*)a->v_w[0], (const float*)a->v_w[1]}, {(const float*)a->v_b[0], (const float*)a->v_b[1]}};
    AdPtr2 O = {{(const float*)a->o_w[0], (const float*)a->o_w[1]}, {(const float*)a->o_b[0], (const float*)a->o_b[1]}};
    const long ob = (long)B * AD;
    hipLaunchKernelGGL(adapter_gemv_kernel, dim3(AD / 4, 2), dim3(256), 0, stream, V, (const float*)w.ctx, c_as, c_bs, AD / G, B, w.vcat, ob, (long)AD);
    hipLaunchKernelGGL(adapter_gemv_kernel, dim3(AD / 4, 2), dim3(256), 0, stream, O, (const float*)w.vcat, ob, (long)AD, AD, B,
                       (float*)a->out_f32, ob, (long)AD);
  }
  return check_launch("carel_adapter_forward");
}

extern "C" int carel_adapter_backward(const carel_adapter_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = ad_check(a, "carel_adapter_backward");
  if (rc) return rc;
  if (!a->x_f32 || !a->d_out_f32 || !a->dx_f32) return set_error(CAREL_ERR_ARG, "carel_adapter_backward: null x / d_out / dx");
  if (a->mode == 0)
    for (int i = 0; i < 2; ++i)
      if (!a->v_w[i] || !a->o_w[i]) return set_error(CAREL_ERR_ARG, "carel_adapter_backward: raw mode needs v_w / o_w");
  const int B = a->batch, S = a->seq_len, G = a->heads, nv = 2 * G;
  AdWork w = ad_carve((float*)a->work, B, S, G);
  const long ob = (long)B * AD;
  const float* dctx = (const float*)a->d_out_f32;
  long d_as = ob, d_bs = AD;
  if (a->mode == 0) {
    AdPtr2 O = {{(const float*)a->o_w[0], (const float*)a->o_w[1]}, {nullptr, nullptr}};
    AdPtr2 V = {{(const float*)a->v_w[0], (const float*)a->v_w[1]}, {nullptr, nullptr}};
    gemvT(O, (const float*)a->d_out_f32, ob, (long)AD, B, 1, 1.0f, w.dvcat, ob, (long)AD, w.part, stream);
    gemvT(V, (const float*)w.dvcat, ob, (long)AD, B, G, 1.0f, w.dctx, (long)B * G * AD, (long)G * AD, w.part, stream);
    dctx = w.dctx; d_as = (long)B * G * AD; d_bs = (long)G * AD;
  }
  const float* x = (const float*)a->x_f32;
  AD_NV_SWITCH(nv, hipLaunchKernelGGL(adapter_rowdot_kernel<NV>, dim3(S / RD_ROWS, B), dim3(256), 0, stream, x, S, B, dctx, d_as, d_bs, G, w.sc));
  AD_NV_SWITCH(nv, hipLaunchKernelGGL(adapter_dzdh_kernel<NV>, dim3(S / DZ_ROWS, a->batch_padded), dim3(192), 0, stream, S, B, G, a->mode,
                                      (const float*)w.p, (const float*)w.sc, dctx, d_as, d_bs, (const float*)a->u, (float*)a->dx_f32));
  return check_launch("carel_adapter_backward");
}

extern "C" int64_t carel_adapter_wgrad_workspace_floats(int32_t batch, int32_t heads) {
  if (batch < 1 || heads < 1) return 0;
  return (int64_t)adwg_carve(nullptr, batch, heads).total;
}

extern "C" int carel_adapter_backward_weights(const carel_adapter_args* a, const carel_adapter_wgrad_args* g, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "carel_adapter_backward_weights";
  int rc = ad_check(a, who);
  if (rc) return rc;
  if (!g) return set_error(CAREL_ERR_ARG, "%s: null gradient args", who);
  if (!g->work) return set_error(CAREL_ERR_ARG, "%s: null work", who);
  if (g->accumulate != 0 && g->accumulate != 1) return set_error(CAREL_ERR_ARG, "%s: accumulate must be 0 or 1", who);
  if (!a->x_f32) return set_error(CAREL_ERR_ARG, "%s: null x", who);
  const bool raw = a->mode == 0;
  if (raw && !a->d_out_f32) return set_error(CAREL_ERR_ARG, "%s: raw mode needs d_out", who);
  for (int i = 0; i < 2; ++i) {
    if (!a->query[i] || !a->k_w[i]) return set_error(CAREL_ERR_ARG, "%s: null query / k_w", who);
    if (!g->d_q_w[i] || !g->d_q_b[i] || !g->d_k_w[i] || !g->d_k_b[i]) return set_error(CAREL_ERR_ARG, "%s: null d_q_* / d_k_*", who);
    if (raw && (!g->d_v_w[i] || !g->d_v_b[i] || !g->d_o_w[i] || !g->d_o_b[i])) return set_error(CAREL_ERR_ARG, "%s: raw mode needs d_v_* / d_o_*", who);
    const void* vec[] = {a->query[i], g->d_q_w[i], g->d_k_w[i], raw ? g->d_v_w[i] : nullptr, raw ? g->d_o_w[i] : nullptr};
    for (const void* q : vec)
      if ((uintptr_t)q & 15) return set_error(CAREL_ERR_ARG, "%s: query and the weight-gradient destinations must be 16-byte aligned", who);
  }
  const int B = a->batch, S = a->seq_len, G = a->heads, nv = 2 * G, dh = AD / G;
  AdWork w = ad_carve((float*)a->work, B, S, G);
  AdWgWork gw = adwg_carve((float*)g->work, B, G);
  const float* x = (const float*)a->x_f32;
  hipLaunchKernelGGL(adapter_wgrad_dz_kernel, dim3((nv * B + 3) / 4), dim3(256), 0, stream, nv * B, S, a->mode, (const float*)w.p,
                     (const float*)w.sc, gw.dz);
  // the one pass over H: per-sample partials du_k(b) = sum_s dz[k][b][s] H[b,s], then the samples in ascending order (x 1/sqrt(d))
  AD_NV_SWITCH(nv, hipLaunchKernelGGL(adapter_combine_kernel<NV>, dim3(AD / CB_COLS, B), dim3(256), 0, stream, x, S, B, G, (const float*)gw.dz,
                                      gw.part, (long)B * G * AD, (long)G * AD));
  hipLaunchKernelGGL(adapter_wgrad_dusum_kernel, dim3((nv * AD + 255) / 256), dim3(256), 0, stream, (const float*)gw.part, B, G,
                     1.0f / sqrtf((float)dh), gw.du);
  // dqv[n] = W_k[n,:] . du_head(n)
  AdPtr2 K = {{(const float*)a->k_w[0], (const float*)a->k_w[1]}, {nullptr, nullptr}};
  hipLaunchKernelGGL(adapter_gemv_kernel, dim3(AD / 4, 2), dim3(256), 0, stream, K, (const float*)gw.du, (long)G * AD, 0L, dh, 1, gw.dqv, (long)AD, 0L);
  AdOuterJobs J = {};
  int nj = 0;
  for (int i = 0; i < 2; ++i) {
    AdOuterJob& k = J.j[0]; AdOuterJob& q = J.j[1];
    k.L[i] = w.qv + i * AD; k.R[i] = gw.du + (long)i * G * AD; k.dW[i] = (float*)g->d_k_w[i]; k.db[i] = (float*)g->d_k_b[i];
    q.L[i] = gw.dqv + i * AD; q.R[i] = (const float*)a->query[i]; q.dW[i] = (float*)g->d_q_w[i]; q.db[i] = (float*)g->d_q_b[i];
  }
  J.j[0].nb = 1; J.j[0].seg = dh; J.j[0].bias = 2;
  J.j[1].nb = 1; J.j[1].seg = AD; J.j[1].bias = 1;
  nj = 2;
  if (raw) {
    const long ob = (long)B * AD;
    for (int i = 0; i < 2; ++i) {
      AdOuterJob& o = J.j[2]; AdOuterJob& v = J.j[3];
      o.L[i] = (const float*)a->d_out_f32 + i * ob; o.R[i] = w.vcat + i * ob; o.dW[i] = (float*)g->d_o_w[i]; o.db[i] = (float*)g->d_o_b[i];
      v.L[i] = w.dvcat + i * ob; v.R[i] = w.ctx + (long)i * B * G * AD; v.dW[i] = (float*)g->d_v_w[i]; v.db[i] = (float*)g->d_v_b[i];
    }
    J.j[2].nb = B; J.j[2].seg = AD; J.j[2].bias = 1; J.j[2].l_bs = AD; J.j[2].r_bs = AD;
    J.j[3].nb = B; J.j[3].seg = dh; J.j[3].bias = 1; J.j[3].l_bs = AD; J.j[3].r_bs = (long)G * AD;
    nj = 4;
  }
  hipLaunchKernelGGL(adapter_wgrad_outer_kernel, dim3(AD / OW_ROWS, 2, nj), dim3(192), 0, stream, J, g->accumulate);
  return check_launch(who);
}
