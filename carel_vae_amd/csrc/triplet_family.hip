// The batch triplet loss family of the `sentence_transformers` package (losses.BatchSemiHardTripletLoss, BatchAllTripletLoss,
// BatchHardTripletLoss, BatchHardSoftMarginTripletLoss; chi_sentence_transformer_old.py:33 trains with BatchAllTripletLoss) for
// batches of up to 512 sentences: carel_triplet_loss.  The package is absent here (parity unpinned); the definitions are stated in
// include/carel_hip.h and restated in float64 by tests/triplet_restate.py.  All fp32 (the final sum over the anchors runs in fp64), no
// float atomics: the same inputs give the same bits.  Four launches on the caller's stream:
//   1. triplet_dist_kernel   one workgroup per 32 x 32 tile of the upper triangle of D; every unordered pair {i, j} is computed ONCE and
//                            stored at [i][j] and [j][i], so D is symmetric bit for bit (the gradient divides W[i][j] + W[j][i] by one D[i][j]);
//   2. triplet_mine_kernel   one workgroup per anchor a: row a of D and the labels in LDS; writes row a of W = d (sum of the loss terms) / d D
//                            (only workgroup a writes row a), the anchor's partial loss and its three counts (int32);
//   3. triplet_finish_kernel sums the partial losses and counts, writes the loss, the optional statistics and the scale 1 / denominator;
//   4. triplet_grad_kernel   demb = scale * sum_j c_ij (e_i - e_j)  /  - scale * sum_j (W[i][j] + W[j][i]) e_j, j in index order.
// carel_triplet_semihard (triplet.hip: one workgroup, B <= 64) is untouched.
#include "carel_hip_internal.h"

#include <limits.h>

namespace carel {

constexpr int TF_MAXB = 512;
constexpr int TF_TILE = 32, TF_KC = 64;   // distance tile: 32 x 32 outputs, K chunks of 64
constexpr int TF_GR = 8;                  // gradient tile: 8 rows x 256 columns per workgroup

// workspace (floats): D [B, B] | W [B, B] | partial loss [B] | counts int32 [B, 3] | scale [1] (+ padding)
__host__ __device__ inline long tf_off_w(int B) { return (long)B * B; }
__host__ __device__ inline long tf_off_part(int B) { return 2l * B * B; }
__host__ __device__ inline long tf_off_counts(int B) { return 2l * B * B + B; }
__host__ __device__ inline long tf_off_scale(int B) { return 2l * B * B + 4l * B; }
__host__ __device__ inline long tf_floats(int B) { return 2l * B * B + 4l * B + 4; }

// ---- 1. distances -------------------------------------------------------------------------------------------------------
// EUCLID: d2 = |e_lo|^2 - 2 e_lo.e_hi + |e_hi|^2 (lo < hi), D = 0 where d2 <= 0 and on the diagonal, else sqrt(d2).
// otherwise: D = 1 - e_i.e_j, the diagonal included (the rows are L2-normalised by the caller for the cosine distance).
// Dot products and squared norms are fmaf chains over k = 0 .. H-1 in index order.
template <bool EUCLID>
__global__ __launch_bounds__(256) void triplet_dist_kernel(const float* __restrict__ emb, int B, int H, float* __restrict__ D) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (ti > tj) return;                                  // the lower triangle is the mirror of the upper one
  __shared__ float As[TF_TILE][TF_KC + 1];              // [row][k], rows ti * 32 ..
  __shared__ float Bs[TF_TILE][TF_KC + 1];              // [row][k], rows tj * 32 ..
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;  // outputs (ty + 16 u, tx + 16 v), u, v = 0, 1
  float dot[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, na[2] = {0.f, 0.f}, nb[2] = {0.f, 0.f};
  // the chunk after the one being multiplied is already on its way from global memory, in registers (one tile is a chain of H / 64
  // dependent load -> LDS -> multiply rounds: with the load inside the round the kernel took 45 us at any batch size)
  float ra[TF_KC / 8], rb[TF_KC / 8];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < TF_KC / 8; ++q) {
      const int e = t + 256 * q, r = e / TF_KC, k = k0 + e % TF_KC;
      const int ia = ti * TF_TILE + r, ib = tj * TF_TILE + r;
      ra[q] = (ia < B && k < H) ? emb[(long)ia * H + k] : 0.f;
      rb[q] = (ib < B && k < H) ? emb[(long)ib * H + k] : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < H; k0 += TF_KC) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TF_KC / 8; ++q) {
      const int e = t + 256 * q;
      As[e / TF_KC][e % TF_KC] = ra[q];
      Bs[e / TF_KC][e % TF_KC] = rb[q];
    }
    __syncthreads();
    if (k0 + TF_KC < H) fetch(k0 + TF_KC);
#pragma unroll 8
    for (int kk = 0; kk < TF_KC; ++kk) {
      const float a0 = As[ty][kk], a1 = As[ty + 16][kk], b0 = Bs[tx][kk], b1 = Bs[tx + 16][kk];
      dot[0][0] = fmaf(a0, b0, dot[0][0]); dot[0][1] = fmaf(a0, b1, dot[0][1]);
      dot[1][0] = fmaf(a1, b0, dot[1][0]); dot[1][1] = fmaf(a1, b1, dot[1][1]);
      if (EUCLID) {
        na[0] = fmaf(a0, a0, na[0]); na[1] = fmaf(a1, a1, na[1]);
        nb[0] = fmaf(b0, b0, nb[0]); nb[1] = fmaf(b1, b1, nb[1]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int i = ti * TF_TILE + ty + 16 * u, j = tj * TF_TILE + tx + 16 * v;
      if (i >= B || j >= B || i > j) continue;          // (i > j only inside a diagonal tile: that pair belongs to another thread)
      float d;
      if (EUCLID) {
        const float d2 = na[u] - 2.0f * dot[u][v] + nb[v];
        d = (i == j || d2 <= 0.f) ? 0.f : sqrtf(d2);
      } else {
        d = 1.0f - dot[u][v];
      }
      D[(long)i * B + j] = d;
      D[(long)j * B + i] = d;
    }
}

// ---- 2. mining ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int block_sum_i(int v, int* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  int s = 0;
  for (int i = 0; i < nw; ++i) s += red[i];
  return s;
}
// the extreme value of a row and its index; among exactly equal values the LOWEST index wins
struct Best { float v; int i; };
template <bool MAX>
__device__ __forceinline__ void best_take(Best& b, float v, int i) {
  if ((MAX ? v > b.v : v < b.v) || (v == b.v && i < b.i)) { b.v = v; b.i = i; }
}
template <bool MAX>
__device__ __forceinline__ Best best_init() { return Best{MAX ? -INFINITY : INFINITY, INT_MAX}; }
template <bool MAX>
__device__ __forceinline__ Best block_best(Best b, float* redv, int* redi) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(b.v, o, 64);
    const int oi = __shfl_xor(b.i, o, 64);
    best_take<MAX>(b, ov, oi);
  }
  __syncthreads();
  if (lane == 0) { redv[w] = b.v; redi[w] = b.i; }
  __syncthreads();
  Best r = best_init<MAX>();
  for (int i = 0; i < nw; ++i) best_take<MAX>(r, redv[i], redi[i]);
  return r;
}

// One anchor per workgroup.  pos(j): same label and j != a; neg(j): another label.  The hinge modes leave integer counts in W
// (exact in f32: at most 511 per entry); the soft-margin mode leaves +-sigmoid(hp - hn).
//   mode 0 (semi-hard): per positive p, the negative is the nearest one farther than p, else the farthest negative, else none (distance 0);
//   mode 1 (all): every (p, n): W[a][p] counts the n with l > 0 (one pass over p), W[a][n] minus the p with l > 0 (one pass over n);
//   mode 2 / 3 (hard, hard soft-margin): hp = max_j (pos ? D : 0), hn = min_j (D + (neg ? 0 : rowmax)).  When hn is taken at a
//     non-negative j (an anchor without a negative) its gradient reaches both D[a][j] and the row maximum, as in the package's formula.
// counts[a] = {positives of a, positives x negatives of a, active terms of a}: active = hinge terms > 0 (mode 1: > 1e-16, the
// package's denominator; mode 3: 1 per anchor).
__global__ __launch_bounds__(256) void triplet_mine_kernel(const float* __restrict__ D, const int* __restrict__ labels, int B, int mode, float margin,
                                                           float* __restrict__ W, float* __restrict__ part, int* __restrict__ counts) {
  __shared__ float d[TF_MAXB];
  __shared__ int lab[TF_MAXB];
  __shared__ int wi[TF_MAXB];
  __shared__ float wf[TF_MAXB];
  __shared__ int plist[TF_MAXB], nlist[TF_MAXB];     // packed positives / negatives of the anchor (indices, ascending)
  __shared__ float pdv[TF_MAXB], ndv[TF_MAXB];       // ... and their distances
  __shared__ int wcnt[2][4];
  __shared__ float redf[16];
  __shared__ int redi[16];
  const int a = blockIdx.x, t = threadIdx.x;
  for (int j = t; j < B; j += 256) { d[j] = D[(long)a * B + j]; lab[j] = labels[j]; wi[j] = 0; wf[j] = 0.f; }
  __syncthreads();
  const int la = lab[a];
  // the positives and the negatives of the anchor, each packed in ascending index order with their distances (ballot + popcount:
  // no atomics, so the order is fixed and the lowest index still wins a tie): the loops below then run over dense lists
  // (at 512 sentences in 8 classes an anchor has ~63 positives: scanning all 512 indices per thread cost 137 us per launch)
  int npos = 0, nneg = 0;
  const int lane = t & 63, wv = t >> 6;
  for (int j0 = 0; j0 < B; j0 += 256) {
    const int j = j0 + t;
    const bool fn = j < B && lab[j] != la, fp = j < B && !fn && j != a;
    const unsigned long long mp = __ballot(fp), mn = __ballot(fn);
    if (lane == 0) { wcnt[0][wv] = __popcll(mp); wcnt[1][wv] = __popcll(mn); }
    __syncthreads();
    int op = npos, on = nneg;
    for (int i = 0; i < wv; ++i) { op += wcnt[0][i]; on += wcnt[1][i]; }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (fp) { const int s = op + __popcll(mp & below); plist[s] = j; pdv[s] = d[j]; }
    if (fn) { const int s = on + __popcll(mn & below); nlist[s] = j; ndv[s] = d[j]; }
    for (int i = 0; i < 4; ++i) { npos += wcnt[0][i]; nneg += wcnt[1][i]; }
    __syncthreads();
  }
  float loss = 0.f;
  int active = 0;
  if (mode == 0) {
    for (int ip = t; ip < npos; ip += 256) {
      const float dap = pdv[ip];
      int i_out = -1, i_in = -1;
      float d_out = 0.f, d_in = 0.f;
#pragma unroll 8
      for (int i = 0; i < nneg; ++i) {                   // (unrolled: the LDS reads of eight negatives are in flight together)
        const float dan = ndv[i];
        if (dan > dap && (i_out < 0 || dan < d_out)) { i_out = i; d_out = dan; }
        if (i_in < 0 || dan > d_in) { i_in = i; d_in = dan; }
      }
      const int isel = i_out >= 0 ? i_out : i_in;
      const float dneg = i_out >= 0 ? d_out : (i_in >= 0 ? d_in : 0.f);
      const float l = dap - dneg + margin;
      if (l > 0.f) {
        loss += l;
        ++active;
        atomicAdd(&wi[plist[ip]], 1);                    // (integer LDS atomics: the order of arrival does not change the sum)
        if (isel >= 0) atomicAdd(&wi[nlist[isel]], -1);
      }
    }
  } else if (mode == 1) {
    for (int ip = t; ip < npos; ip += 256) {
      const float dap = pdv[ip];
      int cnt = 0;
#pragma unroll 8
      for (int i = 0; i < nneg; ++i) {
        const float l = dap - ndv[i] + margin;
        if (l > 0.f) { loss += l; ++cnt; }
        if (l > 1e-16f) ++active;
      }
      wi[plist[ip]] = cnt;
    }
    for (int in = t; in < nneg; in += 256) {
      const float dan = ndv[in];
      int cnt = 0;
#pragma unroll 8
      for (int i = 0; i < npos; ++i) {
        const float l = pdv[i] - dan + margin;           // the expression of the first pass: the same bits, the same decision
        if (l > 0.f) ++cnt;
      }
      wi[nlist[in]] = -cnt;
    }
  } else {
    Best bm = best_init<true>();
    for (int j = t; j < B; j += 256) best_take<true>(bm, d[j], j);
    bm = block_best<true>(bm, redf, redi);
    Best bp = best_init<true>(), bn = best_init<false>();
    for (int j = t; j < B; j += 256) {
      const bool neg = lab[j] != la, pos = !neg && j != a;
      best_take<true>(bp, pos ? d[j] : 0.f, j);
      best_take<false>(bn, d[j] + (neg ? 0.f : bm.v), j);
    }
    bp = block_best<true>(bp, redf, redi);
    bn = block_best<false>(bn, redf, redi);
    if (t == 0) {
      const float x = bp.v - bn.v;
      float w;
      if (mode == 2) {
        const float l = x + margin;
        w = l > 0.f ? 1.f : 0.f;
        if (l > 0.f) { loss = l; active = 1; }
      } else {                                           // log1p(exp(x)) as a stable softplus; its derivative is sigmoid(x)
        const float e = expf(-fabsf(x));
        loss = fmaxf(x, 0.f) + log1pf(e);
        w = x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
        active = 1;
      }
      if (w != 0.f && bm.i < B && bp.i < B && bn.i < B) {   // (a row of NaN distances selects nothing: the indices stay INT_MAX)
        const bool jp_pos = bp.i != a && lab[bp.i] == la;
        if (jp_pos) wf[bp.i] += w;
        wf[bn.i] -= w;
        if (lab[bn.i] == la) wf[bm.i] -= w;
      }
    }
  }
  __syncthreads();
  if (mode <= 1) {
    for (int j = t; j < B; j += 256) W[(long)a * B + j] = (float)wi[j];
  } else {
    for (int j = t; j < B; j += 256) W[(long)a * B + j] = wf[j];
  }
  loss = block_sum(loss, redf);
  active = block_sum_i(active, redi);
  if (t == 0) {
    part[a] = loss;
    counts[3 * a] = npos;
    counts[3 * a + 1] = npos * nneg;
    counts[3 * a + 2] = active;
  }
}

// ---- 3. finish ----------------------------------------------------------------------------------------------------------
// One wave: lane l sums the anchors l, l + 64, ... (fp64 for the losses), then a fixed xor butterfly.
//   mode 0: sum / positive pairs (0 when there is none); mode 1: sum / (active + 1e-16); modes 2, 3: sum / B.
__global__ __launch_bounds__(64) void triplet_finish_kernel(const float* __restrict__ part, const int* __restrict__ counts, int B, int mode,
                                                            float* __restrict__ loss_out, int* __restrict__ stats_out, float* __restrict__ scale) {
  const int lane = threadIdx.x;
  double s = 0.0;
  int c0 = 0, c1 = 0, c2 = 0;
  for (int a = lane; a < B; a += 64) { s += (double)part[a]; c0 += counts[3 * a]; c1 += counts[3 * a + 1]; c2 += counts[3 * a + 2]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64); c2 += __shfl_xor(c2, o, 64);
  }
  if (lane != 0) return;
  double inv;
  if (mode == 0) inv = c0 > 0 ? 1.0 / (double)c0 : 0.0;
  else if (mode == 1) inv = 1.0 / ((double)c2 + 1e-16);
  else inv = 1.0 / (double)B;
  loss_out[0] = (float)(s * inv);
  scale[0] = (float)inv;
  if (stats_out) { stats_out[0] = c0; stats_out[1] = c1; stats_out[2] = c2; }
}

// ---- 4. gradient --------------------------------------------------------------------------------------------------------
// EUCLID: demb[i] = scale * sum_j c_ij (e_i - e_j), c_ij = (W[i][j] + W[j][i]) / D[i][j] where D > 0, else 0;
// otherwise: demb[i] = - scale * sum_j (W[i][j] + W[j][i]) e_j  (j = i included: d (1 - e_i.e_i) / d e_i = -2 e_i).
// One workgroup per (8 rows, 256 columns); the coefficients of the eight rows against every j sit in LDS (16 KB); j runs in index order.
template <bool EUCLID>
__global__ __launch_bounds__(256) void triplet_grad_kernel(const float* __restrict__ emb, const float* __restrict__ D, const float* __restrict__ W,
                                                           const float* __restrict__ scale, int B, int H, float* __restrict__ demb) {
  __shared__ __attribute__((aligned(16))) float c[TF_MAXB][TF_GR];     // [j][row]: the eight coefficients of one j are two 16-byte reads
  const int t = threadIdx.x, i0 = blockIdx.x * TF_GR, k = blockIdx.y * 256 + t;
  const bool kok = k < H;
  float ei[TF_GR], g[TF_GR];
#pragma unroll
  for (int r = 0; r < TF_GR; ++r) {
    ei[r] = (kok && i0 + r < B) ? emb[(long)(i0 + r) * H + k] : 0.f;
    g[r] = 0.f;
  }
  for (int e = t; e < TF_GR * B; e += 256) {              // all B coefficients of the eight rows at once: one round of global latency
    const int r = e / B, j = e - r * B, i = i0 + r;
    float v = 0.f;
    if (i < B) {
      const float w = W[(long)i * B + j] + W[(long)j * B + i];
      if (EUCLID) {
        const float dd = D[(long)i * B + j];
        v = (w != 0.f && dd > 0.f) ? w / dd : 0.f;
      } else {
        v = -w;
      }
    }
    c[j][r] = v;
  }
  __syncthreads();
#pragma unroll 8
  for (int j = 0; j < B; ++j) {                           // (unrolled: eight rows of emb are in flight together)
    const float ej = kok ? emb[(long)j * H + k] : 0.f;
    const float4 c0 = *(const float4*)&c[j][0], c1 = *(const float4*)&c[j][4];
    const float cr[TF_GR] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
    for (int r = 0; r < TF_GR; ++r) g[r] = fmaf(cr[r], EUCLID ? ei[r] - ej : ej, g[r]);
  }
  const float inv = scale[0];
#pragma unroll
  for (int r = 0; r < TF_GR; ++r)
    if (kok && i0 + r < B) demb[(long)(i0 + r) * H + k] = g[r] * inv;
}

}  // namespace carel

using namespace carel;

extern "C" int64_t carel_triplet_workspace_floats(int32_t batch) {
  if (batch < 1 || batch > TF_MAXB) return 0;
  return (int64_t)tf_floats(batch);
}

extern "C" int carel_triplet_loss(const carel_triplet_args* a, void* stream) {
  if (!a) return set_error(CAREL_ERR_ARG, "carel_triplet_loss: null arguments");
  if (!a->emb || !a->labels || !a->loss_out || !a->work) return set_error(CAREL_ERR_ARG, "carel_triplet_loss: null pointer (emb, labels, loss_out, work)");
  if (a->batch < 1 || a->batch > TF_MAXB) return set_error(CAREL_ERR_SHAPE, "carel_triplet_loss: batch %d: must be in 1..%d", a->batch, TF_MAXB);
  if (a->hidden < 1) return set_error(CAREL_ERR_SHAPE, "carel_triplet_loss: hidden %d: must be >= 1", a->hidden);
  if (a->mode < 0 || a->mode > 3) return set_error(CAREL_ERR_ARG, "carel_triplet_loss: mode %d: 0 semi-hard, 1 all, 2 hard, 3 hard soft-margin", a->mode);
  if (a->distance < 0 || a->distance > 1) return set_error(CAREL_ERR_ARG, "carel_triplet_loss: distance %d: 0 Euclidean, 1 one minus dot product", a->distance);
  const int B = a->batch, H = a->hidden;
  hipStream_t s = (hipStream_t)stream;
  const float* emb = (const float*)a->emb;
  float* work = (float*)a->work;
  float* D = work;
  float* W = work + tf_off_w(B);
  float* part = work + tf_off_part(B);
  int* counts = (int*)(work + tf_off_counts(B));
  float* scale = work + tf_off_scale(B);
  const int tiles = (B + TF_TILE - 1) / TF_TILE;
  if (a->distance == 0) hipLaunchKernelGGL(triplet_dist_kernel<true>, dim3(tiles, tiles), dim3(256), 0, s, emb, B, H, D);
  else hipLaunchKernelGGL(triplet_dist_kernel<false>, dim3(tiles, tiles), dim3(256), 0, s, emb, B, H, D);
  hipLaunchKernelGGL(triplet_mine_kernel, dim3(B), dim3(256), 0, s, (const float*)D, (const int*)a->labels, B, a->mode, a->margin, W, part, counts);
  hipLaunchKernelGGL(triplet_finish_kernel, dim3(1), dim3(64), 0, s, (const float*)part, (const int*)counts, B, a->mode, (float*)a->loss_out,
                     (int*)a->stats_out, scale);
  if (a->demb) {
    const dim3 grid((B + TF_GR - 1) / TF_GR, (H + 255) / 256);
    if (a->distance == 0)
      hipLaunchKernelGGL(triplet_grad_kernel<true>, grid, dim3(256), 0, s, emb, (const float*)D, (const float*)W, (const float*)scale, B, H, (float*)a->demb);
    else
      hipLaunchKernelGGL(triplet_grad_kernel<false>, grid, dim3(256), 0, s, emb, (const float*)D, (const float*)W, (const float*)scale, B, H, (float*)a->demb);
  }
  return check_launch("carel_triplet_loss");
}
