// VAE tail of DrlClassifier.forward (drl_classifier_ec_mmd_final_mul.py:202-261) and its backward:
//   pooler (HF BertPooler: tanh(W_p x[:,0] + b_p)) -> 4 latent heads (:312-336) -> reparameterised sample
//   (:345-351, one eps vector shared by the batch, std = exp(log_var)) -> emotion CE (:461-476), cause BCE
//   (:478-492), pair BCE-with-logits + pos_weight (:494-513, replaced by 0 when infinite), RBF-MMD
//   (:231-233), annealed KL (:515-534), decoder softmax + BCE reconstruction (:253-254, :381-387),
//   weighted sum (:256-261).
// Everything is fp32.  The scalar loss and the gradients w.r.t. every tail tensor are produced together
// (the loss is the root of the graph, so backward only rescales them by grad_output).
#include "carel_hip_internal.h"
#include "mmd_device.h"
#include "hsic_device.h"
#include "rowvec_device.h"
#include "tail_device.h"

namespace carel {

#define TAIL_STAMP(i) do { if (a.prof && threadIdx.x == 0) a.prof[i] = (long long)wall_clock64(); } while (0)

// ------------------------------------------------------------------------------------------
// Global-batch RBF-MMD for data parallel runs (z_global = every rank's sampled latents): the statistic needs all
// (2n)^2 pairs -- 1 M at 8 x 64 samples -- which one workgroup would chew on for ~0.4 ms.  Here each workgroup takes 32
// rows (8 lanes per row split the partners, streamed through LDS in chunks of 256 rows) and writes its partial sums of
// the three blocks; rows of THIS rank's samples also get d(gscale * mmd)/dz.  tail_core_kernel adds the partials in
// block order.  Feature width padded to CD with zeros (CD = 24: the reference's ec_dim; 32: anything else <= 32).
// ------------------------------------------------------------------------------------------
struct MmdGlobalArgs {
  const float* zg; int n, B, D, rank_stride, row_offset;     // n samples per side in total, B per rank
  float alpha, eps, gscale;
  float* part;      // [gridDim.x][4]: s11, s22, s12
  float* dz;        // [B][2D] (local rows)
};
template <int CD>
__global__ __launch_bounds__(256) void mmd_global_kernel(MmdGlobalArgs a) {
  constexpr int CH = 256, ZS = CD + 1;
  __shared__ float zc[CH * ZS];
  __shared__ float nc[CH];
  __shared__ float red[64];
  const int t = threadIdx.x, grp = t & 7;
  const int n = a.n, n2 = 2 * n, D = a.D, D2 = 2 * D;
  auto zrow = [&](int r) -> const float* {               // row r of Z = [all emotion samples ; all cause samples]
    const int side = r >= n, s = r - side * n;
    return a.zg + (long)(s / a.B) * a.rank_stride + (long)(s % a.B) * D2 + side * D;
  };
  const int i = blockIdx.x * 32 + (t >> 3);
  const bool live = i < n2;
  float zi[CD], g[CD];
  float ni = 0.f;
  {
    const float* zp = zrow(live ? i : 0);
#pragma unroll
    for (int k = 0; k < CD; ++k) { zi[k] = (k < D) ? zp[k] : 0.f; g[k] = 0.f; ni = fmaf(zi[k], zi[k], ni); }
  }
  const bool i1 = i < n;
  const int si = i - (i1 ? 0 : n);
  const bool local = live && si >= a.row_offset && si < a.row_offset + a.B;
  const float a00 = (float)(1.0 / ((double)n * (n - 1))), a01 = (float)(-1.0 / ((double)n * n));
  float s11 = 0.f, s22 = 0.f, s12 = 0.f;
  for (int c0 = 0; c0 < n2; c0 += CH) {
    const int cn = min(CH, n2 - c0);
    __syncthreads();
    for (int e = t; e < cn * CD; e += 256) {
      const int r = e / CD, k = e - r * CD;
      zc[r * ZS + k] = (k < D) ? zrow(c0 + r)[k] : 0.f;
    }
    __syncthreads();
    for (int r = t; r < cn; r += 256) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < CD; ++k) s = fmaf(zc[r * ZS + k], zc[r * ZS + k], s);
      nc[r] = s;
    }
    __syncthreads();
    if (live) {
      for (int jj = grp; jj < cn; jj += 8) {
        const int j = c0 + jj;
        if (j == i) continue;
        float zj[CD], dot = 0.f;
#pragma unroll
        for (int k = 0; k < CD; ++k) { zj[k] = zc[jj * ZS + k]; dot = fmaf(zi[k], zj[k], dot); }
        const float d2 = ni + nc[jj] - 2.0f * dot;
        const float e = expf(-a.alpha * (a.eps + fabsf(d2)));
        const bool j1 = j < n;
        if (i1 && j1) s11 += e; else if (!i1 && !j1) s22 += e; else if (i1 && !j1) s12 += e;
        if (local) {
          const float dcs = (d2 > 0.f) ? a.alpha * e : ((d2 < 0.f) ? -a.alpha * e : 0.f);
          const float coef = -4.0f * ((i1 == j1) ? a00 : a01) * dcs * a.gscale;
#pragma unroll
          for (int k = 0; k < CD; ++k) g[k] = fmaf(coef, zi[k] - zj[k], g[k]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CD; ++k) {
    float v = g[k];
    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
    if (local && grp == 0 && k < D) a.dz[(long)(si - a.row_offset) * D2 + (i1 ? 0 : D) + k] = v;
  }
  __syncthreads();
  s11 = block_sum(s11, red);
  s22 = block_sum(s22, red + 16);
  s12 = block_sum(s12, red + 32);
  if (t == 0) { a.part[blockIdx.x * 4] = s11; a.part[blockIdx.x * 4 + 1] = s22; a.part[blockIdx.x * 4 + 2] = s12; }
}

static long long* g_tail_prof = nullptr;
// tuning hook (carel_gemm_set_variant(210 / 211)): the single-workgroup loss kernel (~50 us on ONE CU) on the library's low-priority side stream
// while the reconstruction decoder's passes (~100 us, 186 workgroups) run on the caller's stream, joined before the two results meet
CAREL_TUNABLE(int, g_tail_overlap, 1);
#ifdef CAREL_EXPERIMENTS
void tail_overlap_enable(int on) { g_tail_overlap = on ? 1 : 0; }
#endif
struct TailEvents { hipEvent_t fork, join; bool ok; };
static TailEvents* tail_events() {               // two events per device, created on first use and kept for the life of the process
  static TailEvents per_dev[16];
  static bool made[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  if (!made[dev]) {
    TailEvents& t = per_dev[dev];
    t.ok = hipEventCreateWithFlags(&t.fork, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&t.join, hipEventDisableTiming) == hipSuccess;
    made[dev] = true;
  }
  return per_dev[dev].ok ? &per_dev[dev] : nullptr;
}

__global__ __launch_bounds__(1024) void tail_core_kernel(TailCore a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* red = (float*)smem_raw;                 // 64
  float* sc = red + 64;                          // 64 scalars
  const int B = a.B, D = a.D, D2 = 2 * a.D, D4 = 4 * a.D;
  float* zl = sc + 64;                           // [B][2D] sampled latents
  float* dzl = zl + B * D2;                      // [B][2D] gradient accumulator
  float* elog = dzl + B * D2;                    // [B][8] emotion dlogits
  float* gx = elog + B * 8;                      // [B][2]  cause / pair dlogit
  float* mlt = gx + B * 2;                       // [B][4D] dropout multipliers: emotion [D] | cause [D] | pair [2D]
  float* lg = mlt + B * D4;                      // [B][16] head logits: emotion classes, then cause, then pair
  float* hw = lg + B * 16;                       // head weights: emo_w [EC*D], emo_b [EC], cau_w [D], cau_b, pair_w [2D], pair_b
  const HeadLayout L(a.EC, D);
  const int nm = a.z_global ? a.n_global : B;    // samples per side in the MMD
  float* nrm = hw + ((L.n + 3) & ~3);            // [2 nm]
  float* Z = nrm + ((2 * nm + 3) & ~3);          // MMD samples [2 nm][D|1]
  const int zs = D | 1;
  const int t = threadIdx.x;
  TAIL_STAMP(0);

  for (int e = t; e < B * D2; e += blockDim.x) {
    const int b = e / D2, k = e - b * D2;
    const float z = sample_z(a.lat + (long)b * 4 * D, a.eps_e, a.eps_c, D, k);
    zl[e] = z; dzl[e] = 0.f;
    if (a.z) a.z[e] = z;
  }
  fill_dropout_mults(a, mlt, 0, B, t, blockDim.x);
  load_head_weights(a, L, hw, t, blockDim.x);
  __syncthreads();
  // ---- MMD samples: rows [0,nm) emotion, [nm,2nm) cause   (not needed when mmd_global_kernel did the statistic)
  for (int e = t; e < (a.mmd_part ? 0 : 2 * nm * D); e += blockDim.x) {
    const int i = e / D, k = e - i * D;
    const int s = i < nm ? i : i - nm, off = i < nm ? 0 : D;
    Z[i * zs + k] = a.z_global ? a.z_global[(long)(s / B) * a.rank_stride + (long)(s % B) * D2 + off + k] : zl[s * D2 + off + k];
  }
  __syncthreads();
  TAIL_STAMP(1);
  float mmd = 0.f;                     // value of the disentanglement statistic (terms[1])
  float dis_term = 0.f;                // its contribution to the loss
  if (a.dis_mode == 0 && a.mmd_part) {
    // mmd_global_kernel's partials; the gradient rows are already computed
    if (t == 0) sc[0] = mmd_from_partials(a, nm);
    __syncthreads();
    mmd = sc[0];
    dis_term = -a.w_mmd * mmd;
    for (int e = t; e < B * D2; e += blockDim.x) dzl[e] += a.dz_mmd[e];
    TAIL_STAMP(2);
  } else if (a.dis_mode == 0) {
    MmdCfg mc; mc.n1 = nm; mc.n2 = nm; mc.d = D; mc.zs = zs; mc.n_alphas = 1; mc.alphas[0] = a.alpha; mc.eps = a.mmd_eps;
    if (!a.z_global && D == 24) {      // the configuration of every reference script: one fused forward + backward sweep
      mmd = mmd_forward_backward_block<24>(mc, Z, nrm, red, -a.w_mmd * a.mmd_grad_scale, dzl, D2);
      dis_term = -a.w_mmd * mmd;
      TAIL_STAMP(2);
    } else {
      mmd = mmd_forward_block(mc, Z, nrm, red, nullptr);
      dis_term = -a.w_mmd * mmd;
      TAIL_STAMP(2);
      // d(-w_mmd * mmd)/dz for the local rows: 8 threads per row
      const int rows = 2 * B;
      const int grp = t & 7;
      for (int base = 0; base < rows; base += blockDim.x / 8) {
        const int rloc = base + (t >> 3);
        float g[32];
        const bool live = rloc < rows;
        if (live) {
          const int side = rloc >= B, bl = rloc - side * B;
          const int i = side * nm + a.row_offset * (a.z_global ? 1 : 0) + bl;
          mmd_backward_row(mc, Z, nrm, i, -a.w_mmd * a.mmd_grad_scale, g, grp, 8);
        } else {
          for (int k = 0; k < D; ++k) g[k] = 0.f;
        }
        for (int k = 0; k < D; ++k) {
          float v = g[k];
          v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
          if (live && grp == 0) { const int side = rloc >= B, bl = rloc - side * B; dzl[bl * D2 + side * D + k] += v; }
        }
      }
    }
  } else if (a.dis_mode == 1) {        // HSIC between the local emotion (rows 0..B) and cause (rows B..2B) samples
    HsicCfg hc; hc.m = B; hc.d = D; hc.xs = zs; hc.inv_sx = 1.0f; hc.inv_sy = 1.0f;
    float* rk = Z + 2 * nm * zs;       // [B] row sums of K, then [B] of L (extra LDS reserved by the host)
    float* rl = rk + B;
    mmd = hsic_forward_block(hc, Z, Z + B * zs, nrm, nrm + B, rk, rl, red);
    dis_term = a.w_mmd * mmd;
    const float tk = red[60], tl = red[61];
    for (int i = t; i < B; i += blockDim.x) {
      float gx[32], gy[32];
      hsic_backward_row(hc, Z, Z + B * zs, nrm, nrm + B, rk, rl, tk, tl, i, a.w_mmd, gx, gy);
      for (int k = 0; k < D; ++k) { dzl[i * D2 + k] += gx[k]; dzl[i * D2 + D + k] += gy[k]; }
    }
  }
  __syncthreads();
  TAIL_STAMP(3);
  // ---- classifier heads: 16 threads per sample, one per logit (emotion classes, cause, pair)
  for (int e = t; e < B * 16; e += blockDim.x) {
    const int b = e >> 4, h = e & 15;
    if (h < a.EC + 2) lg[e] = head_logit(a, L, hw, zl, mlt, b, h);
  }
  float l_emo = 0.f, l_cau = 0.f, l_pair = 0.f, ysum = 0.f;
  if (t < B) ysum = a.pair_labels[t];
  ysum = block_sum(t < B ? ysum : 0.f, red);        // (its barriers also publish lg)
  const float pw = pair_pos_weight(a, ysum);
  for (int b = t; b < B; b += blockDim.x) {          // losses and dlogits of a row in one trip (the pair dlogit waits for `dead`)
    const float* lr = lg + b * 16;
    emo_row<true, true>(a, lr, b, l_emo, elog + b * 8);
    l_cau += cau_row_loss(a, lr, b);
    gx[b * 2] = cau_row_dlogit(a, lr, b);
    l_pair += pair_row_loss(a, lr, b, pw);
  }
  l_emo = block_sum(l_emo, red) / B;
  l_cau = block_sum(l_cau, red) / B;
  l_pair = block_sum(l_pair, red) / B;
  const bool dead = isinf(l_pair);
  if (dead) l_pair = 0.f;
  for (int b = t; b < B; b += blockDim.x) gx[b * 2 + 1] = pair_row_dlogit(a, lg + b * 16, b, pw, dead);
  __syncthreads();
  TAIL_STAMP(4);
  // ---- KL (:525-534) and its direct gradient on lat
  float kle = 0.f, klc = 0.f;
  for (int e = t; e < B * D; e += blockDim.x) {
    const int b = e / D, k = e - b * D;
    kl_row(a, b, k, kle, klc);
  }
  kle = block_sum(kle, red) / B * a.kl_w;
  klc = block_sum(klc, red) / B * a.kl_w;
  TAIL_STAMP(5);
  // ---- dz from the three heads, and the head parameter gradients
  for (int e = t; e < B * D2; e += blockDim.x) {
    const int b = e / D2, k = e - b * D2;
    dzl[e] += heads_dz(a, L, hw, mlt, elog, gx, b, k);
  }
  TAIL_STAMP(6);
  // parameter gradients: thread per parameter element, loop over the batch (fixed order)
  for (int e = t; e < L.n; e += blockDim.x) *head_grad_dst(a, L, e) = head_param_grad(a, L, zl, mlt, elog, gx, e, B);
  __syncthreads();
  TAIL_STAMP(7);
  for (int e = t; e < B * D2; e += blockDim.x) a.dz[e] = dzl[e];
  if (t == 0) write_terms(a, mmd, dis_term, l_emo, l_cau, l_pair, kle, klc, dead);
}

// CD2 > 0: 2*ec_dim known at compile time (weights stay in registers); CD2 == 0: generic run-time width.
// Thread t: entry tj = t % DEC_J of the chunk, sample group g = t / DEC_J (G = blockDim.x / DEC_J groups, each a
// contiguous range of ceil(B/G) samples): 4x the waves of a thread-per-entry layout, bow values prefetched four samples
// ahead.  Per-group results are combined in fixed order, so the outputs are run-to-run reproducible.
template <int PASS, int CD2>
__global__ __launch_bounds__(DEC_J * DEC_MAXG) void decoder_kernel(DecArgs a) {
  const int D2 = CD2 ? CD2 : a.D2;
  const int ws = D2 + 1;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* zl = (float*)smem_raw;                       // [B][D2]
  float* red = zl + a.B * D2;                         // 16
  float* wl = red + 16;                               // [DEC_J][D2+1] weights of the chunk
  float* tile = wl + DEC_J * ws;                      // [B][DEC_J] per-(sample, entry) values (pass 3: dlogits)
  float* tile2 = tile + a.B * DEC_J;                  // pass 2: second tile; pass 3: [G-1][DEC_J][D2+1] dW partials + [G-1][DEC_J] db
  const int t = threadIdx.x, nthr = blockDim.x, G = nthr / DEC_J;
  const int tj = t & (DEC_J - 1), g = t / DEC_J;
  const int j0 = blockIdx.x * DEC_J, j = j0 + tj;
  const bool live = j < a.V;
  const int Bg = (a.B + G - 1) / G, b0 = g * Bg, b1 = min(a.B, b0 + Bg);
  for (int e = t; e < a.B * D2; e += nthr) zl[e] = a.z[e];
  {   // coalesced load of the chunk's weights, then each thread takes its row
    const int nrow = min(DEC_J, a.V - j0);
    for (int e = t; e < nrow * D2; e += nthr) { const int r = e / D2, k = e - r * D2; wl[r * ws + k] = a.w[(long)j0 * D2 + e]; }
  }
  __syncthreads();
  float wr[CD2 ? CD2 : DEC_MAXD2];
  _Pragma("unroll") for (int k = 0; k < D2; ++k) wr[k] = live ? wl[tj * ws + k] : 0.f;
  const float bias = live ? a.b[j] : 0.f;
  const int lane = t & 63, wv = t >> 6, nwv = nthr >> 6;
  if (PASS == 1) {
    for (int b = b0; b < b1; ++b) tile[b * DEC_J + tj] = live ? dec_logit<CD2>(wr, zl + b * D2, D2, bias) : -INFINITY;
    __syncthreads();
    for (int b = wv; b < a.B; b += nwv) {
      const float x0 = tile[b * DEC_J + lane], x1 = tile[b * DEC_J + 64 + lane];
      const float m = wave_max(fmaxf(x0, x1));
      const float s2 = wave_sum(expf(x0 - m) + expf(x1 - m));            // exp(-inf - m) = 0 for dead entries
      if (lane == 0) { a.part[((long)blockIdx.x * a.B + b) * 2] = m; a.part[((long)blockIdx.x * a.B + b) * 2 + 1] = s2; }
    }
  } else if (PASS == 2) {
    for (int bb = b0; bb < b1; bb += 4) {
      float bw[4];
      _Pragma("unroll") for (int u = 0; u < 4; ++u) bw[u] = (live && bb + u < b1) ? a.bow[(long)(bb + u) * a.V + j] : 0.f;
      _Pragma("unroll") for (int u = 0; u < 4; ++u) {
        const int b = bb + u;
        if (b < b1) {
          float le = 0.f, dt = 0.f;
          if (live) {
            const float lp = dec_logit<CD2>(wr, zl + b * D2, D2, bias) - a.rowstat[b * 4] - a.rowstat[b * 4 + 1];
            dec_loss_dot(lp, dec_target(a, bw[u]), le, dt);
          }
          tile[b * DEC_J + tj] = le; tile2[b * DEC_J + tj] = dt;
        }
      }
    }
    __syncthreads();
    for (int b = wv; b < a.B; b += nwv) {
      const float le = wave_sum(tile[b * DEC_J + lane] + tile[b * DEC_J + 64 + lane]);
      const float dt = wave_sum(tile2[b * DEC_J + lane] + tile2[b * DEC_J + 64 + lane]);
      if (lane == 0) { a.part[((long)blockIdx.x * a.B + b) * 2] = le; a.part[((long)blockIdx.x * a.B + b) * 2 + 1] = dt; }
    }
  } else {
    float dwr[CD2 ? CD2 : DEC_MAXD2];
    _Pragma("unroll") for (int k = 0; k < D2; ++k) dwr[k] = 0.f;
    float dbj = 0.f;
    for (int bb = b0; bb < b1; bb += 4) {
      float bw[4];
      _Pragma("unroll") for (int u = 0; u < 4; ++u) bw[u] = (live && bb + u < b1) ? a.bow[(long)(bb + u) * a.V + j] : 0.f;
      _Pragma("unroll") for (int u = 0; u < 4; ++u) {
        const int b = bb + u;
        if (b < b1) {
          float gg = 0.f;
          if (live) {
            const float lp = dec_logit<CD2>(wr, zl + b * D2, D2, bias) - a.rowstat[b * 4] - a.rowstat[b * 4 + 1];
            const float p = expf(lp);
            const float gp = bce_dprob(p, dec_target(a, bw[u]));
            gg = p * (gp - a.rowstat[b * 4 + 2]) * a.gscale;
            _Pragma("unroll") for (int k = 0; k < D2; ++k) dwr[k] = fmaf(gg, zl[b * D2 + k], dwr[k]);
            dbj += gg;
          }
          tile[b * DEC_J + tj] = gg;
        }
      }
    }
    float* dwp = tile2;                               // [G-1][DEC_J][ws]
    float* dbp = dwp + (G - 1) * DEC_J * ws;          // [G-1][DEC_J]
    if (g > 0) {
      _Pragma("unroll") for (int k = 0; k < D2; ++k) dwp[((g - 1) * DEC_J + tj) * ws + k] = dwr[k];
      dbp[(g - 1) * DEC_J + tj] = dbj;
    }
    __syncthreads();
    if (g == 0 && live) {
      for (int q = 0; q < G - 1; ++q) {               // fixed order: group 0 + group 1 + ...
        _Pragma("unroll") for (int k = 0; k < D2; ++k) dwr[k] += dwp[(q * DEC_J + tj) * ws + k];
        dbj += dbp[q * DEC_J + tj];
      }
      _Pragma("unroll") for (int k = 0; k < D2; ++k) a.dw[(long)j * D2 + k] = dwr[k];
      a.db[j] = dbj;
    }
    // dz_part[chunk][b][k] = sum_{j in chunk} dlogit[b][j] * W[j][k]
    for (int e = t; e < a.B * D2; e += nthr) {
      const int b = e / D2, k = e - b * D2;
      const int nrow = min(DEC_J, a.V - j0);
      float s = 0.f;
      for (int jj = 0; jj < nrow; ++jj) s = fmaf(tile[b * DEC_J + jj], wl[jj * ws + k], s);
      a.dz_part[(long)blockIdx.x * a.B * D2 + e] = s;
    }
  }
}

// combine pass-1 partials -> rowstat[b] = {M, log L}; pass-2 partials -> rowstat[b][2] = dot, [3] = row loss.
// One wave per sample (lanes over chunks).
__global__ __launch_bounds__(256) void decoder_combine_kernel(const float* __restrict__ part, int chunks, int B, int pass,
                                                              float* __restrict__ rowstat) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  if (pass == 1) {
    float m = -INFINITY;
    for (int c = lane; c < chunks; c += 64) m = fmaxf(m, part[((long)c * B + b) * 2]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < chunks; c += 64) s += part[((long)c * B + b) * 2 + 1] * expf(part[((long)c * B + b) * 2] - m);
    s = wave_sum(s);
    if (lane == 0) { rowstat[b * 4] = m; rowstat[b * 4 + 1] = logf(s); }
  } else {
    float le = 0.f, dt = 0.f;
    for (int c = lane; c < chunks; c += 64) { le += part[((long)c * B + b) * 2]; dt += part[((long)c * B + b) * 2 + 1]; }
    le = wave_sum(le); dt = wave_sum(dt);
    if (lane == 0) { rowstat[b * 4 + 2] = dt; rowstat[b * 4 + 3] = le; }
  }
}
// rec = sum_b rowloss[b] / (B V); terms[7] = rec, terms[8] = terms[0] + rec
__global__ __launch_bounds__(256) void decoder_total_kernel(const float* __restrict__ rowstat, int B, float inv_bv, float* __restrict__ terms) {
  __shared__ float red[16];
  float tot = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) tot += rowstat[b * 4 + 3];
  tot = block_sum(tot, red);
  if (threadIdx.x == 0) { terms[7] = tot * inv_bv; terms[8] = terms[0] + tot * inv_bv; }
}

// out[c] = sum_p parts[p][c]: 16 columns x 16 part-lanes per block, fixed order
__global__ __launch_bounds__(256) void reduce_parts16_kernel(const float* __restrict__ parts, float* __restrict__ out, int n, int nparts) {
  __shared__ float lds[256];
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float s = 0.f;
  if (c < n) for (int p = rl; p < nparts; p += 16) s += parts[(long)p * n + c];
  lds[threadIdx.x] = s;
  __syncthreads();
  if (rl == 0 && c < n) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += lds[r * 16 + cl];
    out[c] = t;
  }
}

// dlat = dlat_direct + [dz_e, dz_e*eps_e*exp(lv_e), dz_c, dz_c*eps_c*exp(lv_c)], dz = dz_core + sum_chunks dz_part
__global__ __launch_bounds__(256) void tail_dlat_kernel(const float* __restrict__ dz_core, const float* __restrict__ dz_part, int chunks,
                                                        const float* __restrict__ dlat_direct, const float* __restrict__ lat,
                                                        const float* __restrict__ eps_e, const float* __restrict__ eps_c, int B, int D,
                                                        float gout, float* __restrict__ dlat) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * 2 * D) return;
  const int b = e / (2 * D), k = e - b * 2 * D;
  float g = dz_core[e];
  for (int c = 0; c < chunks; ++c) g += dz_part[(long)c * B * 2 * D + e];
  const int side = k >= D, kk = k - side * D;
  const float* row = lat + (long)b * 4 * D;
  const float ep = side ? eps_c[kk] : eps_e[kk];
  const float lv = row[(2 * side + 1) * D + kk];
  dlat[(long)b * 4 * D + 2 * side * D + kk] = (dlat_direct[(long)b * 4 * D + 2 * side * D + kk] + g) * gout;
  dlat[(long)b * 4 * D + (2 * side + 1) * D + kk] = (dlat_direct[(long)b * 4 * D + (2 * side + 1) * D + kk] + g * ep * expf(lv)) * gout;
}

// z = [mu_e + eps_e * exp(lv_e) | mu_c + eps_c * exp(lv_c)]   (sample_prior :345-351)
__global__ __launch_bounds__(256) void sample_z_kernel(const float* __restrict__ lat, const float* __restrict__ eps_e,
                                                       const float* __restrict__ eps_c, int B, int D, float* __restrict__ z) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * 2 * D) return;
  const int b = e / (2 * D), k = e - b * 2 * D;
  z[e] = sample_z(lat + (long)b * 4 * D, eps_e, eps_c, D, k);
}

// The pair head on one sampled pair of latents, stated once for pair_prob_kernel and pair_draws_kernel: component k of the emotion and of
// the cause sample (mu + eps * e^lv, with ex = e^lv) enters the logit in this order, and the logit becomes a probability by pair_sigmoid.
__device__ __forceinline__ float pair_logit_step(float s, float w_e, float mu_e, float eps_e, float ex_e, float w_c, float mu_c, float eps_c,
                                                 float ex_c) {
  s = fmaf(w_e, mu_e + eps_e * ex_e, s);
  return fmaf(w_c, mu_c + eps_c * ex_c, s);
}
__device__ __forceinline__ float pair_sigmoid(float s) { return 1.0f / (1.0f + expf(-s)); }

// eval-mode pair probabilities (get_pair_preds :265-282): sigmoid(w . [mu_e + eps_e e^lv_e, mu_c + eps_c e^lv_c] + b)
__global__ __launch_bounds__(256) void pair_prob_kernel(const float* __restrict__ lat, const float* __restrict__ eps_e,
                                                        const float* __restrict__ eps_c, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int B, int D, float* __restrict__ prob) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float* row = lat + (long)b * 4 * D;
  float s = bias[0];
  for (int k = 0; k < D; ++k)
    s = pair_logit_step(s, w[k], row[k], eps_e[k], expf(row[D + k]), w[D + k], row[2 * D + k], eps_c[k], expf(row[3 * D + k]));
  prob[b] = pair_sigmoid(s);
}

// Many noise draws over the same latents (carel_pair_probs_draws): the encoder, pooler / adapters and latent heads are deterministic in
// eval mode, so a re-evaluation with fresh noise (get_pair_preds, quirk Q6) only changes eps_e / eps_c.  A workgroup owns PD_ROWS rows
// (one per thread: the row's mu and e^lv stay in registers) and blockIdx.y walks the draws in slices of PD_SLICE, whose noise and the
// pair head's weights sit in LDS (every lane reads the same word: a broadcast).  Per (draw, row) the arithmetic is pair_prob_kernel's.
// Counts (TP / FP / FN per draw and group, prediction = prob > 0.5) are integers end to end: a ballot of the predictions per wave and
// draw, popcounts against the wave's label and group masks (formed once), one LDS slot per wave, then one integer global add per
// (workgroup, draw, group, kind) into counts that the host entry has zeroed on the same stream.  Integer sums do not depend on order.
constexpr int PD_ROWS = 256;
constexpr int PD_SLICE = 32;
constexpr int PD_MAXG = 8;

template <int DP>      // ec_dim rounded up to a multiple of 8: the extent of the register arrays
__global__ __launch_bounds__(PD_ROWS) void pair_draws_kernel(const float* __restrict__ lat, const float* __restrict__ eps_e,
                                                             const float* __restrict__ eps_c, const float* __restrict__ w,
                                                             const float* __restrict__ bias, int n, int D, int K, float* __restrict__ prob,
                                                             const float* __restrict__ labels, const int* __restrict__ groups, int G,
                                                             int* __restrict__ counts) {
  __shared__ float s_ee[PD_SLICE * DP], s_ec[PD_SLICE * DP], s_w[2 * DP];
  __shared__ int s_cnt[PD_ROWS / 64][PD_SLICE][3 * PD_MAXG];
  const int t = threadIdx.x, b = blockIdx.x * PD_ROWS + t, k0 = blockIdx.y * PD_SLICE;
  const int nd = K - k0 < PD_SLICE ? K - k0 : PD_SLICE;
  for (int i = t; i < nd * D; i += PD_ROWS) {
    const int d = i / D, k = i - d * D;
    s_ee[d * DP + k] = eps_e[(long)(k0 + d) * D + k];
    s_ec[d * DP + k] = eps_c[(long)(k0 + d) * D + k];
  }
  for (int i = t; i < 2 * D; i += PD_ROWS) s_w[i < D ? i : DP + (i - D)] = w[i];
  const bool valid = b < n;
  const float* row = lat + (long)(valid ? b : n - 1) * 4 * D;      // threads past the last row stay for the ballots; they write nothing
  float mu_e[DP], ex_e[DP], mu_c[DP], ex_c[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const bool in = k < D;
    mu_e[k] = in ? row[k] : 0.0f;
    ex_e[k] = in ? expf(row[D + k]) : 0.0f;
    mu_c[k] = in ? row[2 * D + k] : 0.0f;
    ex_c[k] = in ? expf(row[3 * D + k]) : 0.0f;
  }
  const float b0 = bias[0];
  unsigned long long pm = 0, gm[PD_MAXG];
  if (counts) {
    pm = __ballot(valid && labels[b] == 1.0f);
    const int grp = valid ? (groups ? groups[b] : 0) : -1;           // an id outside [0, G) is in no group
#pragma unroll
    for (int g = 0; g < PD_MAXG; ++g) gm[g] = __ballot(grp == g);
  }
  __syncthreads();
  const int wave = t >> 6, lane = t & 63;
  for (int d = 0; d < nd; ++d) {
    float s = b0;
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (k < D) s = pair_logit_step(s, s_w[k], mu_e[k], s_ee[d * DP + k], ex_e[k], s_w[DP + k], mu_c[k], s_ec[d * DP + k], ex_c[k]);
    const float p = pair_sigmoid(s);
    if (prob && valid) prob[(long)(k0 + d) * n + b] = p;
    if (counts) {
      const unsigned long long pr = __ballot(valid && p > 0.5f);      // .round() of a probability: exactly 0.5 predicts 0 (ref :282)
      if (lane == 0) {
#pragma unroll
        for (int g = 0; g < PD_MAXG; ++g)
          if (g < G) {
            s_cnt[wave][d][3 * g + 0] = __popcll(pr & pm & gm[g]);
            s_cnt[wave][d][3 * g + 1] = __popcll(pr & ~pm & gm[g]);
            s_cnt[wave][d][3 * g + 2] = __popcll(~pr & pm & gm[g]);
          }
      }
    }
  }
  if (!counts) return;
  __syncthreads();
  for (int i = t; i < nd * 3 * G; i += PD_ROWS) {
    const int d = i / (3 * G), j = i - d * 3 * G;
    int c = 0;
    for (int wv = 0; wv < PD_ROWS / 64; ++wv) c += s_cnt[wv][d][j];
    if (c) atomicAdd(&counts[(long)(k0 + d) * 3 * G + j], c);
  }
}

// ------------------------------------------------------------------------------------------
// Batch-tiled form of the loss step (carel_tail_losses_tiled): the work of tail_core_kernel from "classifier heads" through
// "parameter gradients" gridded over slabs of TT_R rows, and the three decoder passes with the batch walked in tiles of TB rows.
// LDS per workgroup does not depend on the batch.  Whatever couples the batch (the pair label sum behind pos_weight, the divisor
// of the means, the "dead" decision on the batch-mean pair loss) is that of the whole batch, which takes two phases:
//   phase 1  logits (kept in the workspace), per-row losses and KL -> per-slab partial sums; dlat_direct
//   phase 2  totals formed in slab order by every workgroup (same bits everywhere), dlogits, dz = heads + dz_mmd, per-slab
//            partials of the head parameter gradients; workgroup 0 also writes terms[0..6] and pair_dead
//   tail_head_grads_kernel adds the parameter-gradient partials in slab order.
// The MMD is mmd_global_kernel's (on the batch's own z, or on z_global), its partials added in block order in double as on
// tail_core_kernel's mmd_part branch.  No atomics: every sum has an order fixed by indices.
// ------------------------------------------------------------------------------------------
constexpr int TT_R = 64;            // rows per slab
constexpr int TT_THREADS = 256;
constexpr int TT_MAX_B = 1024;
constexpr int TT_MAX_SLABS = TT_MAX_B / TT_R;
constexpr int TT_MAX_NHW = HeadLayout(8, 32).n;                // head parameters at ec_dim 32, 8 classes

struct TailTiled {
  TailCore c;              // c.z: the batch's sampled latents, already written by sample_z_kernel
  float* lg;               // [B][16] head logits (phase 1 -> phase 2)
  float* spart;            // [slabs][8]: sums over the slab's rows of the emotion, cause, pair losses and the two KL sums
  float* hpart;            // [slabs][n_hw] head parameter gradients of the slab's rows
};

template <int PHASE>
__global__ __launch_bounds__(TT_THREADS) void tail_heads_kernel(TailTiled q) {
  const TailCore& a = q.c;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* red = (float*)smem_raw;                 // 64
  const int B = a.B, D = a.D, D2 = 2 * a.D, D4 = 4 * a.D;
  float* zl = red + 64;                          // [R][2D] sampled latents of the slab
  float* mlt = zl + TT_R * D2;                   // [R][4D] dropout multipliers: emotion [D] | cause [D] | pair [2D]
  float* lg = mlt + TT_R * D4;                   // [R][16] head logits
  float* elog = lg + TT_R * 16;                  // [R][8] emotion dlogits
  float* gx = elog + TT_R * 8;                   // [R][2] cause / pair dlogit
  float* hw = gx + TT_R * 2;                     // head weights, as in tail_core_kernel
  const HeadLayout L(a.EC, D);
  const int t = threadIdx.x;
  const int r0 = blockIdx.x * TT_R, nr = min(TT_R, B - r0);       // this slab: rows r0 .. r0 + nr - 1
  const int nslab = gridDim.x;

  for (int e = t; e < nr * D2; e += TT_THREADS) zl[e] = a.z[(long)r0 * D2 + e];
  fill_dropout_mults(a, mlt, r0, nr, t, TT_THREADS);
  load_head_weights(a, L, hw, t, TT_THREADS);
  if (PHASE == 2) for (int e = t; e < nr * 16; e += TT_THREADS) lg[e] = q.lg[(long)r0 * 16 + e];
  __syncthreads();
  if (PHASE == 1) {
    // ---- classifier heads: 16 threads per sample, one per logit (emotion classes, cause, pair)
    for (int e = t; e < nr * 16; e += TT_THREADS) {
      const float s = head_logit(a, L, hw, zl, mlt, e >> 4, e & 15);
      lg[e] = s;
      q.lg[(long)r0 * 16 + e] = s;
    }
  }
  // ---- pos_weight of the whole batch: label sum in an order fixed by the index (or the override)
  float ysum = 0.f;
  for (int b = t; b < B; b += TT_THREADS) ysum += a.pair_labels[b];
  ysum = block_sum(ysum, red);                    // (its barriers also publish lg)
  const float pw = pair_pos_weight(a, ysum);
  if (PHASE == 1) {
    float l_emo = 0.f, l_cau = 0.f, l_pair = 0.f;
    for (int b = t; b < nr; b += TT_THREADS) head_row_losses(a, lg + b * 16, r0 + b, pw, l_emo, l_cau, l_pair);
    l_emo = block_sum(l_emo, red);
    l_cau = block_sum(l_cau, red);
    l_pair = block_sum(l_pair, red);
    // ---- KL (:525-534) and its direct gradient on lat
    float kle = 0.f, klc = 0.f;
    for (int e = t; e < nr * D; e += TT_THREADS) kl_row(a, r0 + e / D, e % D, kle, klc);
    kle = block_sum(kle, red);
    klc = block_sum(klc, red);
    if (t == 0) {
      float* sp = q.spart + blockIdx.x * 8;
      sp[0] = l_emo; sp[1] = l_cau; sp[2] = l_pair; sp[3] = kle; sp[4] = klc;
    }
    return;
  }
  // ---- phase 2: the totals of the batch in slab order (every thread of every workgroup forms the same sums)
  float l_emo = 0.f, l_cau = 0.f, l_pair = 0.f, kle = 0.f, klc = 0.f;
  for (int s = 0; s < nslab; ++s) {
    const float* sp = q.spart + s * 8;
    l_emo += sp[0]; l_cau += sp[1]; l_pair += sp[2]; kle += sp[3]; klc += sp[4];
  }
  l_emo = l_emo / B; l_cau = l_cau / B; l_pair = l_pair / B;
  kle = kle / B * a.kl_w; klc = klc / B * a.kl_w;
  const bool dead = isinf(l_pair);
  if (dead) l_pair = 0.f;
  for (int b = t; b < nr; b += TT_THREADS) head_row_dlogits(a, lg + b * 16, r0 + b, pw, dead, elog + b * 8, gx + b * 2);
  __syncthreads();
  // ---- dz = d(statistic)/dz + the three heads
  for (int e = t; e < nr * D2; e += TT_THREADS) {
    const int b = e / D2, k = e - b * D2;
    const float g = heads_dz(a, L, hw, mlt, elog, gx, b, k);
    const float g0 = a.dz_mmd ? a.dz_mmd[(long)r0 * D2 + e] : 0.f;
    a.dz[(long)r0 * D2 + e] = g0 + g;
  }
  // ---- head parameter gradients of this slab's rows: thread per parameter element, rows in order
  float* hp = q.hpart + (long)blockIdx.x * L.n;
  for (int e = t; e < L.n; e += TT_THREADS) hp[e] = head_param_grad(a, L, zl, mlt, elog, gx, e, nr);
  if (blockIdx.x == 0 && t == 0) {
    float mmd = 0.f, dis_term = 0.f;
    if (a.dis_mode == 0) {
      mmd = mmd_from_partials(a, a.z_global ? a.n_global : B);
      dis_term = -a.w_mmd * mmd;
    }
    write_terms(a, mmd, dis_term, l_emo, l_cau, l_pair, kle, klc, dead);
  }
}

// head parameter gradients = the slabs' partials added in slab order
__global__ __launch_bounds__(TT_THREADS) void tail_head_grads_kernel(TailTiled q, int nslab) {
  const TailCore& a = q.c;
  const HeadLayout L(a.EC, a.D);
  for (int e = threadIdx.x; e < L.n; e += TT_THREADS) {
    float s = 0.f;
    for (int p = 0; p < nslab; ++p) s += q.hpart[(long)p * L.n + e];
    *head_grad_dst(a, L, e) = s;
  }
}

// The decoder's three passes with the batch walked in tiles of TB rows (TB a multiple of DEC_MAXG; DEC_MAXG sample groups, each
// a contiguous quarter of the tile).  LDS: z [TB][D2], the chunk's weights, one [TB][DEC_J] tile (two in pass 2).  Passes 1 and 2:
// grid (chunk, batch tile), partials indexed by row as in decoder_kernel.  Pass 3: one workgroup per chunk walks the tiles in
// ascending order with dW[j] / db[j] of its sample group in registers, dz_part[chunk][b] written per row; at the end the groups'
// sums are added in group order (through the weight image, which is free by then).
template <int PASS, int CD2>
__global__ __launch_bounds__(DEC_J * DEC_MAXG) void decoder_tiled_kernel(DecArgs a, int TB) {
  const int D2 = CD2 ? CD2 : a.D2;
  const int ws = D2 + 1;
  constexpr int G = DEC_MAXG, NTHR = DEC_J * DEC_MAXG;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* zl = (float*)smem_raw;                       // [TB][D2]
  float* wl = zl + TB * D2;                           // [DEC_J][D2+1] weights of the chunk
  float* tile = wl + ((DEC_J * ws + 3) & ~3);         // [TB][DEC_J] per-(sample, entry) values (pass 3: dlogits)
  float* tile2 = tile + TB * DEC_J;                   // pass 2: second tile
  const int t = threadIdx.x;
  const int tj = t & (DEC_J - 1), g = t / DEC_J;
  const int j0 = blockIdx.x * DEC_J, j = j0 + tj;
  const bool live = j < a.V;
  const int nrow = min(DEC_J, a.V - j0);
  const int Rg = TB / G, lb0 = g * Rg;                // this group's rows of a tile: lb0 .. lb0 + Rg - 1
  for (int e = t; e < nrow * D2; e += NTHR) { const int r = e / D2, k = e - r * D2; wl[r * ws + k] = a.w[(long)j0 * D2 + e]; }
  __syncthreads();
  float wr[CD2 ? CD2 : DEC_MAXD2];
  _Pragma("unroll") for (int k = 0; k < D2; ++k) wr[k] = live ? wl[tj * ws + k] : 0.f;
  const float bias = live ? a.b[j] : 0.f;
  const int lane = t & 63, wv = t >> 6, nwv = NTHR >> 6;
  if (PASS == 1 || PASS == 2) {
    const int t0 = blockIdx.y * TB, nb = min(TB, a.B - t0);
    const int lb1 = min(nb, lb0 + Rg);
    for (int e = t; e < nb * D2; e += NTHR) zl[e] = a.z[(long)t0 * D2 + e];
    __syncthreads();
    if (PASS == 1) {
      for (int lb = lb0; lb < lb1; ++lb) tile[lb * DEC_J + tj] = live ? dec_logit<CD2>(wr, zl + lb * D2, D2, bias) : -INFINITY;
      __syncthreads();
      for (int lb = wv; lb < nb; lb += nwv) {
        const float x0 = tile[lb * DEC_J + lane], x1 = tile[lb * DEC_J + 64 + lane];
        const float m = wave_max(fmaxf(x0, x1));
        const float s2 = wave_sum(expf(x0 - m) + expf(x1 - m));            // exp(-inf - m) = 0 for dead entries
        if (lane == 0) { a.part[((long)blockIdx.x * a.B + t0 + lb) * 2] = m; a.part[((long)blockIdx.x * a.B + t0 + lb) * 2 + 1] = s2; }
      }
    } else {
      for (int bb = lb0; bb < lb1; bb += 4) {
        float bw[4];
        _Pragma("unroll") for (int u = 0; u < 4; ++u) bw[u] = (live && bb + u < lb1) ? a.bow[(long)(t0 + bb + u) * a.V + j] : 0.f;
        _Pragma("unroll") for (int u = 0; u < 4; ++u) {
          const int lb = bb + u;
          if (lb < lb1) {
            float le = 0.f, dt = 0.f;
            if (live) {
              const float lp = dec_logit<CD2>(wr, zl + lb * D2, D2, bias) - a.rowstat[(t0 + lb) * 4] - a.rowstat[(t0 + lb) * 4 + 1];
              dec_loss_dot(lp, dec_target(a, bw[u]), le, dt);
            }
            tile[lb * DEC_J + tj] = le; tile2[lb * DEC_J + tj] = dt;
          }
        }
      }
      __syncthreads();
      for (int lb = wv; lb < nb; lb += nwv) {
        const float le = wave_sum(tile[lb * DEC_J + lane] + tile[lb * DEC_J + 64 + lane]);
        const float dt = wave_sum(tile2[lb * DEC_J + lane] + tile2[lb * DEC_J + 64 + lane]);
        if (lane == 0) { a.part[((long)blockIdx.x * a.B + t0 + lb) * 2] = le; a.part[((long)blockIdx.x * a.B + t0 + lb) * 2 + 1] = dt; }
      }
    }
  } else {
    float dwr[CD2 ? CD2 : DEC_MAXD2];
    _Pragma("unroll") for (int k = 0; k < D2; ++k) dwr[k] = 0.f;
    float dbj = 0.f;
    for (int t0 = 0; t0 < a.B; t0 += TB) {
      const int nb = min(TB, a.B - t0);
      const int lb1 = min(nb, lb0 + Rg);
      __syncthreads();                                  // the previous tile's dz_part sweep has read zl / tile
      for (int e = t; e < nb * D2; e += NTHR) zl[e] = a.z[(long)t0 * D2 + e];
      __syncthreads();
      for (int bb = lb0; bb < lb1; bb += 4) {
        float bw[4];
        _Pragma("unroll") for (int u = 0; u < 4; ++u) bw[u] = (live && bb + u < lb1) ? a.bow[(long)(t0 + bb + u) * a.V + j] : 0.f;
        _Pragma("unroll") for (int u = 0; u < 4; ++u) {
          const int lb = bb + u;
          if (lb < lb1) {
            float gg = 0.f;
            if (live) {
              const float lp = dec_logit<CD2>(wr, zl + lb * D2, D2, bias) - a.rowstat[(t0 + lb) * 4] - a.rowstat[(t0 + lb) * 4 + 1];
              const float p = expf(lp);
              const float gp = bce_dprob(p, dec_target(a, bw[u]));
              gg = p * (gp - a.rowstat[(t0 + lb) * 4 + 2]) * a.gscale;
              _Pragma("unroll") for (int k = 0; k < D2; ++k) dwr[k] = fmaf(gg, zl[lb * D2 + k], dwr[k]);
              dbj += gg;
            }
            tile[lb * DEC_J + tj] = gg;
          }
        }
      }
      __syncthreads();
      // dz_part[chunk][b][k] = sum_{j in chunk} dlogit[b][j] * W[j][k]
      for (int e = t; e < nb * D2; e += NTHR) {
        const int lb = e / D2, k = e - lb * D2;
        float s = 0.f;
        for (int jj = 0; jj < nrow; ++jj) s = fmaf(tile[lb * DEC_J + jj], wl[jj * ws + k], s);
        a.dz_part[((long)blockIdx.x * a.B + t0) * D2 + e] = s;
      }
    }
    for (int p = 1; p < G; ++p) {                       // fixed order: group 0 + group 1 + ...
      __syncthreads();
      if (g == p) {
        _Pragma("unroll") for (int k = 0; k < D2; ++k) wl[tj * ws + k] = dwr[k];
        tile[tj] = dbj;
      }
      __syncthreads();
      if (g == 0) {
        _Pragma("unroll") for (int k = 0; k < D2; ++k) dwr[k] += wl[tj * ws + k];
        dbj += tile[tj];
      }
    }
    if (g == 0 && live) {
      _Pragma("unroll") for (int k = 0; k < D2; ++k) a.dw[(long)j * D2 + k] = dwr[k];
      a.db[j] = dbj;
    }
  }
}

}  // namespace carel

using namespace carel;

static size_t align_up(size_t x) { return (x + 63) & ~(size_t)63; }
constexpr int MMD_MAX_BLOCKS = 1024;          // mmd_global_kernel: 32 rows per block -> up to 16 384 samples per side
constexpr size_t TAIL_LDS_MAX = 160 * 1024;   // LDS of one CU

struct TailWork {     // carve-up of the caller's f32 workspace
  float* dz_core; float* dlat_direct; float* dlat; float* dpooled; float* dpre; float* part; float* rowstat; float* dz_part;
  float* dcls; float* dgpart; float* pair_dead; float* mmd_part; float* dz_mmd;
  float* tt_lg; float* tt_spart; float* tt_hpart;      // carel_tail_losses_tiled only; appended, so every earlier offset is where it was
  size_t total;
};
static TailWork carve(float* base, int B, int D, int V) {
  TailWork w; size_t o = 0;
  const int chunks = (V + DEC_J - 1) / DEC_J;
  auto take = [&](size_t n) { float* p = base ? base + o : nullptr; o += align_up(n); return p; };
  w.dz_core = take((size_t)B * 2 * D); w.dlat_direct = take((size_t)B * 4 * D); w.dlat = take((size_t)B * 4 * D);
  w.dpooled = take((size_t)B * TH); w.dpre = take((size_t)B * TH); w.part = take((size_t)chunks * B * 2);
  w.rowstat = take((size_t)B * 4); w.dz_part = take((size_t)chunks * B * 2 * D); w.dcls = take((size_t)B * TH);
  w.dgpart = take((size_t)((TH + DG_CHUNK - 1) / DG_CHUNK) * B * TH);
  w.pair_dead = take(16);
  w.mmd_part = take(4 * MMD_MAX_BLOCKS); w.dz_mmd = take((size_t)B * 2 * D);
  w.tt_lg = take((size_t)B * 16); w.tt_spart = take((size_t)TT_MAX_SLABS * 8); w.tt_hpart = take((size_t)TT_MAX_SLABS * TT_MAX_NHW);
  w.total = o;
  return w;
}

extern "C" int64_t carel_tail_workspace_floats(int32_t batch, int32_t ec_dim, int32_t bow_dim) {
  return (int64_t)carve(nullptr, batch, ec_dim, bow_dim).total;
}

static int tail_check(const carel_tail_args* a, const char* who) {
  if (!a) return set_error(CAREL_ERR_ARG, "%s: null args", who);
  if (a->hidden != TH) return set_error(CAREL_ERR_SHAPE, "%s: hidden must be %d", who, TH);
  if (a->batch < 1 || a->seq_len < 1) return set_error(CAREL_ERR_SHAPE, "%s: bad batch/seq_len", who);
  if (a->ec_dim < 1 || a->ec_dim > 32 || a->e_classes < 1 || a->e_classes > 8)
    return set_error(CAREL_ERR_SHAPE, "%s: ec_dim must be <= 32 and e_num_class <= 8", who);
  if (!a->x_last_f32 || !a->pooler_w || !a->pooler_b || !a->pooled || !a->lat)
    return set_error(CAREL_ERR_ARG, "%s: null tensor", who);
  for (int i = 0; i < 4; ++i) if (!a->head_w[i] || !a->head_b[i]) return set_error(CAREL_ERR_ARG, "%s: null latent head", who);
  return CAREL_OK;
}

// pooler + latent heads:  pooled [B,768], lat [B,4D]
extern "C" int carel_tail_latents(const carel_tail_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = tail_check(a, "carel_tail_latents");
  if (rc) return rc;
  auto sample_groups = [&](int ncols) { int g = (4096 + ncols - 1) / ncols;      /* ~4 k waves: each walks its samples four at a time, one round trip to memory per trip */ const int mx = (a->batch + 3) / 4; g = g > mx ? mx : g; return g < 1 ? 1 : g; };
  const int N = 4 * a->ec_dim;
  if (a->head_in_f32) {      // sentence adapters: the emotion heads read block 0, the cause heads block 1 (no pooler)
    const int N2 = 2 * a->ec_dim;
    for (int side = 0; side < 2; ++side) {
      PtrSet4 hp; for (int i = 0; i < 4; ++i) { hp.w[i] = nullptr; hp.b[i] = nullptr; }
      for (int i = 0; i < 2; ++i) { hp.w[i] = (const float*)a->head_w[2 * side + i]; hp.b[i] = (const float*)a->head_b[2 * side + i]; }
      hipLaunchKernelGGL(rowvec_linear_kernel<0>, dim3((N2 + 3) / 4, sample_groups(N2)), dim3(256), 0, stream,
                         (const float*)a->head_in_f32 + (long)side * a->batch * TH, (long)TH, (const int*)nullptr, a->batch, N2, a->ec_dim, hp,
                         (float*)a->lat + side * N2, (long)N);
    }
  } else {
    PtrSet4 pp; for (int i = 0; i < 4; ++i) { pp.w[i] = nullptr; pp.b[i] = nullptr; }
    pp.w[0] = (const float*)a->pooler_w; pp.b[0] = (const float*)a->pooler_b;
    hipLaunchKernelGGL(rowvec_linear_kernel<1>, dim3(TH / 4, sample_groups(TH)), dim3(256), 0, stream, (const float*)a->x_last_f32,
                       (long)a->seq_len * TH, (const int*)a->cls_rows, a->batch, TH, TH, pp, (float*)a->pooled, (long)TH);
    PtrSet4 hp; for (int i = 0; i < 4; ++i) { hp.w[i] = (const float*)a->head_w[i]; hp.b[i] = (const float*)a->head_b[i]; }
    hipLaunchKernelGGL(rowvec_linear_kernel<0>, dim3((N + 3) / 4, sample_groups(N)), dim3(256), 0, stream, (const float*)a->pooled, (long)TH,
                       (const int*)nullptr, a->batch, N, a->ec_dim, hp, (float*)a->lat, (long)N);
  }
  if (a->eps_e && a->eps_c && a->z)      // the sampled embeddings, for callers that exchange them before carel_tail_losses (data parallel)
    hipLaunchKernelGGL(sample_z_kernel, dim3((a->batch * 2 * a->ec_dim + 255) / 256), dim3(256), 0, stream, (const float*)a->lat,
                       (const float*)a->eps_e, (const float*)a->eps_c, a->batch, a->ec_dim, (float*)a->z);
  return check_launch("tail latents");
}

extern "C" int carel_pair_probs(const void* lat, const void* eps_e, const void* eps_c, const void* pair_w, const void* pair_b,
                                int32_t batch, int32_t ec_dim, void* prob, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!lat || !eps_e || !eps_c || !pair_w || !pair_b || !prob || batch < 1) return set_error(CAREL_ERR_ARG, "carel_pair_probs: bad arguments");
  hipLaunchKernelGGL(pair_prob_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, (const float*)lat, (const float*)eps_e,
                     (const float*)eps_c, (const float*)pair_w, (const float*)pair_b, batch, ec_dim, (float*)prob);
  return check_launch("pair_prob_kernel");
}

extern "C" int carel_pair_probs_draws(const void* lat, const void* eps_e, const void* eps_c, const void* pair_w, const void* pair_b,
                                      int32_t n, int32_t ec_dim, int32_t n_draws, void* prob, const void* labels, const void* groups,
                                      int32_t n_groups, void* counts, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "carel_pair_probs_draws";
  if (!lat || !eps_e || !eps_c || !pair_w || !pair_b) return set_error(CAREL_ERR_ARG, "%s: null tensor", who);
  if (!prob && !counts) return set_error(CAREL_ERR_ARG, "%s: neither prob nor counts to write", who);
  if (counts && !labels) return set_error(CAREL_ERR_ARG, "%s: counts need labels", who);
  if (n < 1 || n_draws < 1) return set_error(CAREL_ERR_SHAPE, "%s: n and n_draws must be >= 1", who);
  if (ec_dim < 1 || ec_dim > 32) return set_error(CAREL_ERR_SHAPE, "%s: ec_dim must be in 1..32", who);
  if (n_groups < 1 || n_groups > PD_MAXG) return set_error(CAREL_ERR_SHAPE, "%s: n_groups must be in 1..%d", who, PD_MAXG);
  const long slices = ((long)n_draws + PD_SLICE - 1) / PD_SLICE;
  if (slices > 65535) return set_error(CAREL_ERR_SHAPE, "%s: at most %d draws per call", who, 65535 * PD_SLICE);
  if (counts) {
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_draws * n_groups * 3 * sizeof(int), stream);
    if (e != hipSuccess) return set_error(CAREL_ERR_HIP, "%s: memset: %s", who, hipGetErrorString(e));
  }
  const dim3 grid((n + PD_ROWS - 1) / PD_ROWS, (unsigned)slices);
#define CAREL_PD_LAUNCH(DP)                                                                                                             \
  hipLaunchKernelGGL(pair_draws_kernel<DP>, grid, dim3(PD_ROWS), 0, stream, (const float*)lat, (const float*)eps_e, (const float*)eps_c, \
                     (const float*)pair_w, (const float*)pair_b, n, ec_dim, n_draws, (float*)prob, (const float*)labels,                  \
                     (const int*)groups, n_groups, (int*)counts)
  if (ec_dim <= 8) CAREL_PD_LAUNCH(8);
  else if (ec_dim <= 16) CAREL_PD_LAUNCH(16);
  else if (ec_dim <= 24) CAREL_PD_LAUNCH(24);
  else CAREL_PD_LAUNCH(32);
#undef CAREL_PD_LAUNCH
  return check_launch("pair_draws_kernel");
}

// ---- the two LDS plans of carel_tail_losses (its batch limit), shared with carel_tail_batch_limit
// loss kernel (one workgroup): the whole batch's z, dz, dropout multipliers, logits, dlogits and the MMD / HSIC rows (nm per side)
static size_t tail_core_lds_bytes(int B, int D, int EC, int nm) {
  const int n_hw = HeadLayout(EC, D).n;
  return sizeof(float) * (64 + 64 + (size_t)2 * B * 2 * D + (size_t)B * 8 + (size_t)B * 2 + (size_t)B * 4 * D + (size_t)B * 16 +
                          ((n_hw + 3) & ~3) + ((2 * nm + 3) & ~3) + (size_t)2 * nm * (D | 1) + 2 * (size_t)B);
}
// decoder: z + red + weights + tile [B][DEC_J] (+ pass 2: second tile; pass 3: the other groups' dW/db partials)
struct DecPlan { int G; size_t lds1, lds2, lds3, ldsmax; };
static DecPlan tail_decoder_plan(int B, int D) {
  DecPlan p;
  const size_t lds0 = sizeof(float) * ((size_t)B * 2 * D + 16 + (size_t)DEC_J * (2 * D + 1) + (size_t)B * DEC_J);
  int G = DEC_MAXG;
  auto lds3_of = [&](int g) { return lds0 + sizeof(float) * (size_t)(g - 1) * DEC_J * (2 * D + 2); };
  while (G > 1 && (lds3_of(G) > TAIL_LDS_MAX || (B + G - 1) / G < 4)) G >>= 1;
  p.G = G; p.lds1 = lds0; p.lds2 = lds0 + sizeof(float) * (size_t)B * DEC_J; p.lds3 = lds3_of(G);
  p.ldsmax = p.lds2 > p.lds3 ? p.lds2 : p.lds3;
  return p;
}

extern "C" int32_t carel_tail_batch_limit(int32_t ec_dim, int32_t e_classes) {
  if (ec_dim < 1 || ec_dim > 32 || e_classes < 1 || e_classes > 8 || 2 * ec_dim > DEC_MAXD2) return 0;
  int B = 1;       // both plans grow with the batch: the largest accepted one is the last before the first refusal
  while (tail_core_lds_bytes(B + 1, ec_dim, e_classes, B + 1) <= TAIL_LDS_MAX && tail_decoder_plan(B + 1, ec_dim).ldsmax <= TAIL_LDS_MAX) ++B;
  return B >= 2 ? B : 0;
}

// ---- launches common to carel_tail_losses and carel_tail_losses_tiled
// the global-batch MMD kernel on nm samples per side: block partials -> w.mmd_part, d/dz of the local rows -> w.dz_mmd
static int launch_mmd_global(TailCore& c, const TailWork& w, const float* zg, int nm, int rank_stride, int row_offset, hipStream_t stream) {
  MmdGlobalArgs g;
  g.zg = zg; g.n = nm; g.B = c.B; g.D = c.D; g.rank_stride = rank_stride; g.row_offset = row_offset;
  g.alpha = c.alpha; g.eps = c.mmd_eps; g.gscale = -c.w_mmd * c.mmd_grad_scale; g.part = w.mmd_part; g.dz = w.dz_mmd;
  const int nblk = (2 * nm + 31) / 32;
  if (c.D == 24) hipLaunchKernelGGL(mmd_global_kernel<24>, dim3(nblk), dim3(256), 0, stream, g);
  else hipLaunchKernelGGL(mmd_global_kernel<32>, dim3(nblk), dim3(256), 0, stream, g);
  if (int rc = check_launch("mmd_global_kernel")) return rc;
  c.mmd_part = w.mmd_part; c.mmd_nblk = nblk; c.dz_mmd = w.dz_mmd;
  return CAREL_OK;
}

static DecArgs dec_args(const carel_tail_args* a, const TailWork& w) {
  DecArgs d;
  d.B = a->batch; d.D2 = 2 * a->ec_dim; d.V = a->bow_dim; d.z = (const float*)a->z; d.w = (const float*)a->dec_w; d.b = (const float*)a->dec_b;
  d.bow = (const float*)a->bow; d.ls = a->label_smoothing; d.part = w.part; d.rowstat = w.rowstat; d.dz_part = w.dz_part;
  d.dw = (float*)a->d_dec_w; d.db = (float*)a->d_dec_b; d.gscale = 1.0f / ((float)a->batch * (float)a->bow_dim);
  return d;
}

// the two decoder families: [0] the compile-time width 48 (ec_dim 24), [1] a run-time width; passes 1..3 in each
static void (*const DEC_WG[2][3])(DecArgs) = {{decoder_kernel<1, 48>, decoder_kernel<2, 48>, decoder_kernel<3, 48>},
                                              {decoder_kernel<1, 0>, decoder_kernel<2, 0>, decoder_kernel<3, 0>}};
static void (*const DEC_TILED[2][3])(DecArgs, int) = {{decoder_tiled_kernel<1, 48>, decoder_tiled_kernel<2, 48>, decoder_tiled_kernel<3, 48>},
                                                      {decoder_tiled_kernel<1, 0>, decoder_tiled_kernel<2, 0>, decoder_tiled_kernel<3, 0>}};
// the three passes with the two combines between them.  grid12: passes 1 and 2, grid3: pass 3; lds: per pass; x: the tiled family's TB
template <typename F, typename... X>
static void launch_decoder(F* const (&K)[2][3], const DecArgs& d, dim3 grid12, dim3 grid3, int threads, const size_t (&lds)[3],
                           hipStream_t stream, X... x) {
  F* const (&k)[3] = K[d.D2 == 48 ? 0 : 1];
  const int chunks = (d.V + DEC_J - 1) / DEC_J;
  hipLaunchKernelGGL(k[0], grid12, dim3(threads), lds[0], stream, d, x...);
  hipLaunchKernelGGL(decoder_combine_kernel, dim3((d.B + 3) / 4), dim3(256), 0, stream, (const float*)d.part, chunks, d.B, 1, d.rowstat);
  hipLaunchKernelGGL(k[1], grid12, dim3(threads), lds[1], stream, d, x...);
  hipLaunchKernelGGL(decoder_combine_kernel, dim3((d.B + 3) / 4), dim3(256), 0, stream, (const float*)d.part, chunks, d.B, 2, d.rowstat);
  hipLaunchKernelGGL(k[2], grid3, dim3(threads), lds[2], stream, d, x...);
}

// sum the decoder's per-chunk dz partials into slot 0 (in place is safe: block c only reads column c of every part)
static void launch_dz_reduce(const carel_tail_args* a, const TailWork& w, hipStream_t stream) {
  const int n = a->batch * 2 * a->ec_dim;
  hipLaunchKernelGGL(reduce_parts16_kernel, dim3((n + 15) / 16), dim3(256), 0, stream, (const float*)w.dz_part, w.dz_part, n, (a->bow_dim + DEC_J - 1) / DEC_J);
}
// where the loss kernels and the decoder meet: terms[7..8] (reads terms[0] of the loss kernel), and d(loss)/d lat, unscaled (grad_output
// is applied in carel_tail_backward)
static int launch_tail_close(const carel_tail_args* a, const TailWork& w, float inv_bv, hipStream_t stream) {
  const int B = a->batch, D = a->ec_dim;
  hipLaunchKernelGGL(decoder_total_kernel, dim3(1), dim3(256), 0, stream, (const float*)w.rowstat, B, inv_bv, (float*)a->terms);
  hipLaunchKernelGGL(tail_dlat_kernel, dim3((B * 2 * D + 255) / 256), dim3(256), 0, stream, (const float*)w.dz_core, (const float*)w.dz_part,
                     1, (const float*)w.dlat_direct, (const float*)a->lat, (const float*)a->eps_e, (const float*)a->eps_c, B, D, 1.0f, w.dlat);
  return check_launch("tail_dlat_kernel");
}

// Argument checks and the loss kernel's arguments, common to carel_tail_losses and carel_tail_losses_tiled (`who` names the caller
// in the messages).  Nothing is launched here.
static int tail_losses_prepare(const carel_tail_args* a, const char* who, TailCore& c, TailWork& w) {
  int rc = tail_check(a, who);
  if (rc) return rc;
  const int B = a->batch, D = a->ec_dim, V = a->bow_dim;
  if (V < 1) return set_error(CAREL_ERR_SHAPE, "%s: bow_dim must be positive", who);
  if (2 * D > DEC_MAXD2) return set_error(CAREL_ERR_SHAPE, "%s: 2*ec_dim must be <= %d", who, DEC_MAXD2);
  if (B < 2 && !a->z_global) return set_error(CAREL_ERR_SHAPE, "%s: batch must be >= 2 (MMD divides by n(n-1))", who);
  if (!a->emo_w || !a->emo_b || !a->cau_w || !a->cau_b || !a->pair_w || !a->pair_b || !a->dec_w || !a->dec_b ||
      !a->emo_labels || !a->cau_labels || !a->pair_labels || !a->bow || !a->eps_e || !a->eps_c || !a->z || !a->terms ||
      !a->work || !a->d_emo_w || !a->d_emo_b || !a->d_cau_w || !a->d_cau_b || !a->d_pair_w || !a->d_pair_b || !a->d_dec_w ||
      !a->d_dec_b)
    return set_error(CAREL_ERR_ARG, "%s: null tensor", who);
  w = carve((float*)a->work, B, D, V);
  c.B = B; c.D = D; c.EC = a->e_classes; c.lat = (const float*)a->lat; c.eps_e = (const float*)a->eps_e; c.eps_c = (const float*)a->eps_c;
  c.emo_w = (const float*)a->emo_w; c.emo_b = (const float*)a->emo_b; c.cau_w = (const float*)a->cau_w; c.cau_b = (const float*)a->cau_b;
  c.pair_w = (const float*)a->pair_w; c.pair_b = (const float*)a->pair_b;
  c.emo_labels = (const long*)a->emo_labels; c.cau_labels = (const float*)a->cau_labels; c.pair_labels = (const float*)a->pair_labels;
  c.w_mmd = a->w_mmd; c.w_emo = a->w_emo; c.w_cau = a->w_cau; c.w_pair = a->w_pair; c.kl_w = a->kl_weight; c.ls = a->label_smoothing;
  c.dis_mode = a->dis_mode; c.emo_bce = a->emo_bce;
  if (c.dis_mode < 0 || c.dis_mode > 2) return set_error(CAREL_ERR_ARG, "%s: dis_mode must be 0 (MMD), 1 (HSIC) or 2 (none)", who);
  if (c.emo_bce && a->e_classes != 1) return set_error(CAREL_ERR_ARG, "%s: the BCE emotion head has exactly one logit", who);
  if (c.dis_mode == 1 && a->z_global) return set_error(CAREL_ERR_ARG, "%s: HSIC has no global-batch mode", who);
  c.d_emo = make_dropout(a->drop_seed, 100u, a->drop_p, a->drop_row_offset * (uint32_t)D);
  c.d_cau = make_dropout(a->drop_seed, 101u, a->drop_p, a->drop_row_offset * (uint32_t)D);
  c.d_pair = make_dropout(a->drop_seed, 102u, a->drop_p, a->drop_row_offset * (uint32_t)(2 * D));
  c.alpha = a->mmd_alpha; c.mmd_eps = a->mmd_eps;
  c.label_sum_override = (const float*)a->global_label_sum; c.n_override = (float)a->global_n;
  c.label_sum_ranks = a->global_label_ranks > 1 ? a->global_label_ranks : 1;
  if (c.label_sum_ranks > 1 && a->global_rank_stride <= 0)
    return set_error(CAREL_ERR_ARG, "%s: global_label_ranks > 1 needs global_rank_stride", who);
  c.z_global = (const float*)a->z_global; c.n_global = a->global_n; c.row_offset = a->global_row_offset;
  c.rank_stride = a->global_rank_stride > 0 ? a->global_rank_stride : B * 2 * D;
  if (c.z_global && a->global_rank_stride > 0 && (a->global_rank_stride < B * 2 * D || c.n_global % B))
    return set_error(CAREL_ERR_ARG, "%s: global_rank_stride needs global_n to be a multiple of batch and stride >= batch*2*ec_dim", who);
  c.mmd_grad_scale = a->mmd_grad_scale > 0.f ? a->mmd_grad_scale : 1.f;
  if (c.z_global && (c.n_global < 2 || c.row_offset < 0 || c.row_offset + B > c.n_global))
    return set_error(CAREL_ERR_ARG, "%s: inconsistent global batch description", who);
  c.z = (float*)a->z; c.terms = (float*)a->terms; c.dz = w.dz_core; c.dlat_direct = w.dlat_direct;
  c.d_emo_w = (float*)a->d_emo_w; c.d_emo_b = (float*)a->d_emo_b; c.d_cau_w = (float*)a->d_cau_w; c.d_cau_b = (float*)a->d_cau_b;
  c.d_pair_w = (float*)a->d_pair_w; c.d_pair_b = (float*)a->d_pair_b; c.pair_dead = w.pair_dead;
  c.mmd_part = nullptr; c.mmd_nblk = 0; c.dz_mmd = nullptr; c.prof = nullptr;
  return CAREL_OK;
}

// losses + gradients of everything after the latents.  Needs carel_tail_latents() first.
extern "C" int carel_tail_losses(const carel_tail_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TailCore c; TailWork w;
  int rc = tail_losses_prepare(a, "carel_tail_losses", c, w);
  if (rc) return rc;
  const int B = a->batch, D = a->ec_dim, V = a->bow_dim;
  const int nm = (c.z_global && c.dis_mode != 0) ? c.n_global : B;        // the global-batch MMD runs in its own kernel
  const size_t lds = tail_core_lds_bytes(B, D, a->e_classes, nm);
  if (lds > TAIL_LDS_MAX) return set_error(CAREL_ERR_SHAPE, "carel_tail_losses: batch too large for the single-workgroup tail (%zu B LDS)", lds);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)tail_core_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_error(CAREL_ERR_HIP, "carel_tail_losses: hipFuncSetAttribute: %s", hipGetErrorString(e));
  }
  // The decoder's launch plan.  Together with the check above this is the batch limit of the call (carel_tail_batch_limit): both
  // kernels keep the whole batch in the 160 KB LDS of one CU.
  const int chunks = (V + DEC_J - 1) / DEC_J;
  const DecPlan dp = tail_decoder_plan(B, D);
  if (dp.ldsmax > TAIL_LDS_MAX) return set_error(CAREL_ERR_SHAPE, "carel_tail_losses: batch too large for the decoder kernel (%zu B LDS)", dp.ldsmax);
  if (dp.ldsmax > 64 * 1024) {
    hipError_t e = hipSuccess;
    for (auto& family : DEC_WG)
      for (auto kernel : family)
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dp.ldsmax);
    if (e != hipSuccess) return set_error(CAREL_ERR_HIP, "carel_tail_losses: hipFuncSetAttribute: %s", hipGetErrorString(e));
  }
  c.mmd_part = nullptr; c.mmd_nblk = 0; c.dz_mmd = nullptr;
  // (every shape check comes BEFORE the fork below -- ADVICE r03: an error return between fork and join would leave the side stream un-joined)
  if (c.z_global && c.dis_mode == 0 && (2 * c.n_global + 31) / 32 > MMD_MAX_BLOCKS)
    return set_error(CAREL_ERR_SHAPE, "carel_tail_losses: global batch too large for the MMD partial buffer");
  // The loss kernel and the decoder passes only share their input z and meet again in decoder_total_kernel (terms[0]) and tail_dlat_kernel:
  // fork the former onto the side stream (the profiling hook keeps the serial order)
  hipStream_t core_stream = stream;
  TailEvents* tev = nullptr;
  // after the fork every early return first joins the side stream back into the caller's stream (whatever was enqueued there completes
  // before the caller's next kernel); the fork / join events are one pair per device: carel_tail_losses with serial = 0 is NOT re-entrant
  // per device (two host threads, or two models interleaving calls on one device, must pass serial = 1)
  auto join_on_error = [&](int code) -> int {
    if (tev && core_stream != stream) {
      (void)hipEventRecord(tev->join, core_stream);
      (void)hipStreamWaitEvent(stream, tev->join, 0);
    }
    return code;
  };
  if (g_tail_overlap && !a->serial && !g_tail_prof) {
    hipStream_t side = (hipStream_t)carel_side_stream(0);     // the weight-gradient stream (idle here: the backward pass has not started); a THIRD stream in play made every later kernel slower
    tev = side ? tail_events() : nullptr;
    if (tev) {
      hipLaunchKernelGGL(sample_z_kernel, dim3((B * 2 * D + 255) / 256), dim3(256), 0, stream, c.lat, c.eps_e, c.eps_c, B, D, c.z);
      if (hipEventRecord(tev->fork, stream) != hipSuccess || hipStreamWaitEvent(side, tev->fork, 0) != hipSuccess)
        return set_error(CAREL_ERR_HIP, "carel_tail_losses: event fork failed");
      core_stream = side;
      c.z = nullptr;
    }
  }
  if (c.z_global && c.dis_mode == 0) {
    if ((rc = launch_mmd_global(c, w, c.z_global, c.n_global, c.rank_stride, c.row_offset, core_stream))) return join_on_error(rc);
  }
  c.prof = g_tail_prof;
  hipLaunchKernelGGL(tail_core_kernel, dim3(1), dim3(1024), lds, core_stream, c);
  if ((rc = check_launch("tail_core_kernel"))) return join_on_error(rc);
  if (tev && hipEventRecord(tev->join, core_stream) != hipSuccess) return join_on_error(set_error(CAREL_ERR_HIP, "carel_tail_losses: event record failed"));

  const DecArgs d = dec_args(a, w);
  const size_t dec_lds[3] = {dp.lds1, dp.lds2, dp.lds3};
  launch_decoder(DEC_WG, d, dim3(chunks), dim3(chunks), DEC_J * dp.G, dec_lds, stream);
  if ((rc = check_launch("decoder kernels"))) return join_on_error(rc);
  launch_dz_reduce(a, w, stream);
  if (tev && hipStreamWaitEvent(stream, tev->join, 0) != hipSuccess) return join_on_error(set_error(CAREL_ERR_HIP, "carel_tail_losses: event join failed"));
  return launch_tail_close(a, w, d.gscale, stream);
}

// The batch-tiled form of carel_tail_losses: same contract, same outputs, same workspace carve, same dropout streams, the same
// data-parallel hooks; 2 <= batch <= 1024 (1 with z_global), MMD or no statistic.  LDS per workgroup does not depend on the batch
// and stays below 64 KB.  Everything runs on the caller's stream (nothing here is a one-CU kernel worth hiding), so the call is
// re-entrant.  Every check comes before the first launch.
extern "C" int carel_tail_losses_tiled(const carel_tail_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "carel_tail_losses_tiled";
  if (!a) return set_error(CAREL_ERR_ARG, "%s: null args", who);
  if (a->batch > TT_MAX_B) return set_error(CAREL_ERR_SHAPE, "%s: batch must be <= %d; got %d", who, TT_MAX_B, a->batch);
  TailTiled q; TailWork w;
  TailCore& c = q.c;
  int rc = tail_losses_prepare(a, who, c, w);
  if (rc) return rc;
  const int B = a->batch, D = a->ec_dim, V = a->bow_dim;
  if (c.dis_mode == 1)
    return set_error(CAREL_ERR_SHAPE, "%s: HSIC (dis_mode 1) keeps the single-workgroup limit of carel_tail_losses: batch <= %d at ec_dim %d, "
                     "e_classes %d; got %d", who, (int)carel_tail_batch_limit(D, a->e_classes), D, a->e_classes, B);
  const int nm = c.z_global ? c.n_global : B;        // samples per side of the MMD
  const int nblk = (2 * nm + 31) / 32;
  if (c.dis_mode == 0 && nblk > MMD_MAX_BLOCKS) return set_error(CAREL_ERR_SHAPE, "%s: global batch too large for the MMD partial buffer", who);
  const int nslab = (B + TT_R - 1) / TT_R;
  const int n_hw = HeadLayout(a->e_classes, D).n;
  const size_t lds_h = sizeof(float) * (64 + (size_t)TT_R * (2 * D + 4 * D + 16 + 8 + 2) + ((n_hw + 3) & ~3));
  const int D2 = 2 * D, chunks = (V + DEC_J - 1) / DEC_J;
  auto dec_lds = [&](int tb, int tiles) { return sizeof(float) * ((size_t)tb * D2 + ((DEC_J * (D2 + 1) + 3) & ~3) + (size_t)tiles * tb * DEC_J); };
  const int TB = dec_lds(32, 2) <= 64 * 1024 ? 32 : 16;
  if (lds_h > 64 * 1024 || dec_lds(TB, 2) > 64 * 1024 || nslab > TT_MAX_SLABS || n_hw > TT_MAX_NHW)
    return set_error(CAREL_ERR_SHAPE, "%s: internal tile plan does not fit (ec_dim %d, e_classes %d)", who, D, a->e_classes);
  const int ntile = (B + TB - 1) / TB;
  q.lg = w.tt_lg; q.spart = w.tt_spart; q.hpart = w.tt_hpart;

  hipLaunchKernelGGL(sample_z_kernel, dim3((B * 2 * D + 255) / 256), dim3(256), 0, stream, c.lat, c.eps_e, c.eps_c, B, D, c.z);
  if (c.dis_mode == 0) {
    rc = c.z_global ? launch_mmd_global(c, w, c.z_global, nm, c.rank_stride, c.row_offset, stream)
                    : launch_mmd_global(c, w, c.z, nm, B * 2 * D, 0, stream);          // on the batch's own z
    if (rc) return rc;
  }
  hipLaunchKernelGGL(tail_heads_kernel<1>, dim3(nslab), dim3(TT_THREADS), lds_h, stream, q);
  hipLaunchKernelGGL(tail_heads_kernel<2>, dim3(nslab), dim3(TT_THREADS), lds_h, stream, q);
  hipLaunchKernelGGL(tail_head_grads_kernel, dim3(1), dim3(TT_THREADS), 0, stream, q, nslab);
  if ((rc = check_launch("tail_heads_kernel"))) return rc;

  const DecArgs d = dec_args(a, w);
  const size_t lds_d[3] = {dec_lds(TB, 1), dec_lds(TB, 2), dec_lds(TB, 1)};
  launch_decoder(DEC_TILED, d, dim3(chunks, ntile), dim3(chunks), DEC_J * DEC_MAXG, lds_d, stream, TB);
  if ((rc = check_launch("decoder kernels (tiled)"))) return rc;
  launch_dz_reduce(a, w, stream);
  return launch_tail_close(a, w, d.gscale, stream);
}

// Back-propagate d(loss)/d lat through the latent heads and the pooler into the encoder output.
// grad_out_dev (device f32 scalar, or NULL for 1.0) is the upstream gradient of the loss: it scales dlat
// in carel_tail_backward_dz; the classifier / decoder gradients written by carel_tail_losses are the caller's to
// scale (they are linear in it): the Python models add grad_output x them into .grad with carel_axpy_f32.
// carel_scale_f32 is the in-place form, kept as a tested utility of the C ABI (tests/test_gpu_tail_sweep.py).
extern "C" int carel_scale_f32(void* x, int64_t n, const void* scale_dev, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !scale_dev || n <= 0) return set_error(CAREL_ERR_ARG, "carel_scale_f32: bad arguments");
  long blocks = (n + 255) / 256; if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(scale_inplace_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (float*)x, (long)n, (const float*)scale_dev);
  return check_launch("scale_inplace_kernel");
}

// Bag-of-words targets shipped as (row, column, value) triples (3-30 entries per clause pair against V = 23 771 columns:
// ~10 KB instead of the 6 MB dense block `bow_reps` of ref :829) and expanded on the device.  `trip` = int32 [nnz] rows,
// int32 [nnz] columns, f32 [nnz] values back to back; entries of one batch are distinct (ECPEDataset builds one entry per
// vocabulary word of the pair), so plain stores suffice.
__global__ void bow_scatter_kernel(const int* __restrict__ rows, const int* __restrict__ cols, const float* __restrict__ vals, int nnz,
                                   float* __restrict__ out, int B, int V) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const int r = rows[i], c = cols[i];
  if (r >= 0 && r < B && c >= 0 && c < V) out[(long)r * V + c] = vals[i];
}
extern "C" int carel_bow_expand(const void* trip, int32_t nnz, void* out, int32_t B, int32_t V, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!out || B < 1 || V < 1 || nnz < 0 || (nnz > 0 && !trip)) return set_error(CAREL_ERR_ARG, "carel_bow_expand: bad arguments");
  hipError_t e = hipMemsetAsync(out, 0, (size_t)B * V * 4, stream);
  if (e != hipSuccess) return set_error(CAREL_ERR_HIP, "carel_bow_expand: memset: %s", hipGetErrorString(e));
  if (nnz == 0) return CAREL_OK;
  const int* rows = (const int*)trip;
  hipLaunchKernelGGL(bow_scatter_kernel, dim3((nnz + 255) / 256), dim3(256), 0, stream, rows, rows + nnz, (const float*)(rows + 2 * (long)nnz), nnz,
                     (float*)out, B, V);
  return check_launch("bow_scatter_kernel");
}

extern "C" int64_t carel_tail_pair_dead_offset(int32_t batch, int32_t ec_dim, int32_t bow_dim) {
  TailWork w = carve((float*)nullptr + 1, batch, ec_dim, bow_dim);   // offsets relative to a fake base
  return (int64_t)(w.pair_dead - ((float*)nullptr + 1));
}

extern "C" int carel_tail_profile(void* dev_i64_x16) { g_tail_prof = (long long*)dev_i64_x16; return CAREL_OK; }

extern "C" int carel_tail_backward(const carel_tail_args* a, const void* grad_out_dev, void* stream_) {
  return carel_tail_backward_dz(a, grad_out_dev, nullptr, stream_);
}

// dlat += [dz_e, dz_e*eps_e*exp(lv_e), dz_c, dz_c*eps_c*exp(lv_c)] for an extra gradient dz on the sampled embeddings
__global__ __launch_bounds__(256) void tail_add_dz_kernel(const float* __restrict__ dz, const float* __restrict__ lat,
                                                          const float* __restrict__ eps_e, const float* __restrict__ eps_c, int B, int D,
                                                          float* __restrict__ dlat) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * 2 * D) return;
  const int b = e / (2 * D), k = e - b * 2 * D, side = k >= D, kk = k - side * D;
  const float g = dz[e];
  const float ep = side ? eps_c[kk] : eps_e[kk];
  const float lv = lat[(long)b * 4 * D + (2 * side + 1) * D + kk];
  dlat[(long)b * 4 * D + 2 * side * D + kk] += g;
  dlat[(long)b * 4 * D + (2 * side + 1) * D + kk] += g * ep * expf(lv);
}

extern "C" int carel_tail_backward_dz(const carel_tail_args* a, const void* grad_out_dev, const void* dz_extra, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = tail_check(a, "carel_tail_backward");
  if (rc) return rc;
  if (!a->work || !a->dx_last_f32 || !a->d_pooler_w || !a->d_pooler_b) return set_error(CAREL_ERR_ARG, "carel_tail_backward: null tensor");
  const int B = a->batch, D = a->ec_dim, N = 4 * D;
  TailWork w = carve((float*)a->work, B, D, a->bow_dim);
  if (grad_out_dev) {
    hipLaunchKernelGGL(scale_inplace_kernel, dim3((B * N + 255) / 256), dim3(256), 0, stream, w.dlat, (long)B * N, (const float*)grad_out_dev);
  }
  if (dz_extra) {
    if (!a->lat || !a->eps_e || !a->eps_c) return set_error(CAREL_ERR_ARG, "carel_tail_backward_dz: lat / eps needed");
    hipLaunchKernelGGL(tail_add_dz_kernel, dim3((B * 2 * D + 255) / 256), dim3(256), 0, stream, (const float*)dz_extra, (const float*)a->lat,
                       (const float*)a->eps_e, (const float*)a->eps_c, B, D, w.dlat);
  }
  const int hc = (N + DG_CHUNK - 1) / DG_CHUNK, pc = (TH + DG_CHUNK - 1) / DG_CHUNK;
  const long bt = (long)B * TH;
  if (a->head_in_f32) {      // sentence adapters: d head_in per side; the pooler is unused (zero gradient), dx_last is carel_adapter_backward's
    if (!a->d_head_in_f32) return set_error(CAREL_ERR_ARG, "carel_tail_backward: head_in_f32 needs d_head_in_f32");
    const int N2 = 2 * D, hc2 = (N2 + DG_CHUNK - 1) / DG_CHUNK;
    for (int side = 0; side < 2; ++side) {
      PtrSet4 hp; OutSet4 ho;
      for (int i = 0; i < 4; ++i) { hp.w[i] = nullptr; hp.b[i] = nullptr; ho.w[i] = nullptr; ho.b[i] = nullptr; }
      for (int i = 0; i < 2; ++i) { hp.w[i] = (const float*)a->head_w[2 * side + i]; ho.w[i] = (float*)a->d_head_w[2 * side + i]; ho.b[i] = (float*)a->d_head_b[2 * side + i]; }
      const float* hin = (const float*)a->head_in_f32 + side * bt;
      if (ho.w[0] && ho.w[1])
        hipLaunchKernelGGL(rowvec_wgrad_kernel, dim3((N2 + 3) / 4), dim3(256), 0, stream, (const float*)w.dlat + side * N2, (long)N, hin,
                           (long)TH, (const int*)nullptr, B, N2, D, ho);
      hipLaunchKernelGGL(rowvec_dgrad_kernel<0>, dim3((B + 3) / 4, hc2), dim3(256), 0, stream, (const float*)w.dlat + side * N2, (long)N, B, N2, D, hp,
                         (const float*)nullptr, (float*)nullptr, w.dgpart);
      hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)((bt / 4 + 255) / 256)), dim3(256), 0, stream, (const float*)w.dgpart,
                         (float*)a->d_head_in_f32 + side * bt, bt, hc2);
    }
    (void)hipMemsetAsync(a->d_pooler_w, 0, (size_t)TH * TH * sizeof(float), stream);
    (void)hipMemsetAsync(a->d_pooler_b, 0, (size_t)TH * sizeof(float), stream);
    return check_launch("tail backward (adapter heads)");
  }
  PtrSet4 hp; OutSet4 ho;
  for (int i = 0; i < 4; ++i) { hp.w[i] = (const float*)a->head_w[i]; hp.b[i] = nullptr; ho.w[i] = (float*)a->d_head_w[i]; ho.b[i] = (float*)a->d_head_b[i]; }
  if (ho.w[0] && ho.w[1] && ho.w[2] && ho.w[3])
    hipLaunchKernelGGL(rowvec_wgrad_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, (const float*)w.dlat, (long)N, (const float*)a->pooled,
                       (long)TH, (const int*)nullptr, B, N, D, ho);
  hipLaunchKernelGGL(rowvec_dgrad_kernel<0>, dim3((B + 3) / 4, hc), dim3(256), 0, stream, (const float*)w.dlat, (long)N, B, N, D, hp,
                     (const float*)nullptr, (float*)nullptr, w.dgpart);
  hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)((bt / 4 + 255) / 256)), dim3(256), 0, stream, (const float*)w.dgpart, w.dpooled, bt, hc);
  PtrSet4 pp; OutSet4 po;
  for (int i = 0; i < 4; ++i) { pp.w[i] = nullptr; pp.b[i] = nullptr; po.w[i] = nullptr; po.b[i] = nullptr; }
  pp.w[0] = (const float*)a->pooler_w; po.w[0] = (float*)a->d_pooler_w; po.b[0] = (float*)a->d_pooler_b;
  hipLaunchKernelGGL(rowvec_dgrad_kernel<1>, dim3((B + 3) / 4, pc), dim3(256), 0, stream, (const float*)w.dpooled, (long)TH, B, TH, TH, pp,
                     (const float*)a->pooled, w.dpre, w.dgpart);
  hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)((bt / 4 + 255) / 256)), dim3(256), 0, stream, (const float*)w.dgpart, w.dcls, bt, pc);
  hipLaunchKernelGGL(rowvec_wgrad_kernel, dim3(TH / 4), dim3(256), 0, stream, (const float*)w.dpre, (long)TH, (const float*)a->x_last_f32,
                     (long)a->seq_len * TH, (const int*)a->cls_rows, B, TH, TH, po);
  const size_t dx_rows = a->n_rows > 0 ? (size_t)a->n_rows : (size_t)B * a->seq_len;
  (void)hipMemsetAsync(a->dx_last_f32, 0, dx_rows * TH * sizeof(float), stream);
  hipLaunchKernelGGL(scatter_cls_kernel, dim3(B), dim3(256), 0, stream, (const float*)w.dcls, B, a->seq_len, (const int*)a->cls_rows,
                     (float*)a->dx_last_f32);
  return check_launch("tail backward");
}
