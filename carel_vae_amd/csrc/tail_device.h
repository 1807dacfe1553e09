// The formulas of the VAE tail's loss step, each stated once for its two schedules in tail.hip: the single-workgroup path
// (tail_core_kernel, decoder_kernel) and the batch-tiled one (tail_heads_kernel<1|2>, decoder_tiled_kernel).  The kernels keep
// their own launch geometry, LDS plans and summation grouping; what a row, a logit or a parameter element computes is here, so
// the two paths agree by construction wherever their summation orders do.
#pragma once
#include "carel_hip_internal.h"

namespace carel {

// ---- loss kernels.  lat = [mu_e | lv_e | mu_c | lv_c] (B x 4D)
struct TailCore {
  int B, D, EC;                 // batch, ec_dim (<= 32), emotion classes (<= 8)
  const float* lat;             // [B, 4D]
  const float* eps_e; const float* eps_c;
  const float* emo_w; const float* emo_b;      // [EC, D], [EC]
  const float* cau_w; const float* cau_b;      // [1, D], [1]
  const float* pair_w; const float* pair_b;    // [1, 2D], [1]
  const long* emo_labels; const float* cau_labels; const float* pair_labels;
  float w_mmd, w_emo, w_cau, w_pair, kl_w, ls;
  int dis_mode;                 // 0: -w_mmd * RBF-MMD (ref :231-233); 1: +w_mmd * HSIC (drl_classifier_ec_hsic.py:214); 2: none
  int emo_bce;                  // 1: one-logit sigmoid + BCE emotion head (ec_hsic/ec_vi scripts) instead of the softmax CE
  Dropout d_emo, d_cau, d_pair;                // element index b*D + k (pair: b*2D + k)
  float alpha, mmd_eps;
  const float* label_sum_override; float n_override;   // global-batch pos_weight (DP); null/0 = local
  int label_sum_ranks;          // > 1: the global label sum is the sum of this many floats, rank_stride apart
  const float* z_global; int n_global, row_offset; float mmd_grad_scale;  // global-batch MMD (DP)
  int rank_stride;              // floats between consecutive ranks' blocks of B rows in z_global (B*2D when dense)
  const float* mmd_part; int mmd_nblk; const float* dz_mmd;   // global-batch MMD computed by mmd_global_kernel (else null)
  // outputs
  float* z;                     // [B, 2D]; null = do not write it (the caller's own sample_z_kernel did: overlapped tail)
  float* terms;                 // [16]: 0 partial loss (everything but rec), 1 mmd, 2 emo, 3 cau, 4 pair, 5 kl_e, 6 kl_c
  float* dz;                    // [B, 2D]  d(loss)/dz (without reconstruction)
  float* dlat_direct;           // [B, 4D]  KL part of d(loss)/d lat
  float* d_emo_w; float* d_emo_b; float* d_cau_w; float* d_cau_b; float* d_pair_w; float* d_pair_b;
  float* pair_dead;             // [1]: 1.0 if the pair loss was replaced by 0 (ref :510-511)
  long long* prof;              // diagnostics (carel_tail_profile): phase time stamps, or null
};

// The head parameters as one image: emo_w [EC*D] at 0, then emo_b [EC], cau_w [D], cau_b, pair_w [2D], pair_b.  The same order
// indexes the LDS copy of the weights, the parameter-gradient loops and the per-slab gradient partials.
struct HeadLayout {
  int eb, cw, cb, pw, pb, n;
  __host__ __device__ __forceinline__ constexpr HeadLayout(int EC, int D) : eb(EC * D), cw(eb + EC), cb(cw + D), pw(cb + 1), pb(pw + 2 * D), n(pb + 1) {}
};

// (nthr: the workgroup's size as the kernel has it -- blockDim.x or a constant -- so that its loops keep their arithmetic)
template <typename N>
__device__ __forceinline__ void load_head_weights(const TailCore& a, const HeadLayout& L, float* hw, int t, N nthr) {
  for (int e = t; e < L.n; e += nthr)
    hw[e] = e < L.eb ? a.emo_w[e] : e < L.cw ? a.emo_b[e - L.eb] : e < L.cb ? a.cau_w[e - L.cw] : e < L.pw ? a.cau_b[0]
          : e < L.pb ? a.pair_w[e - L.pw] : a.pair_b[0];
}
// where parameter element e of the image goes in the caller's gradient tensors
__device__ __forceinline__ float* head_grad_dst(const TailCore& a, const HeadLayout& L, int e) {
  return e < L.eb ? a.d_emo_w + e : e < L.cw ? a.d_emo_b + (e - L.eb) : e < L.cb ? a.d_cau_w + (e - L.cw) : e < L.pw ? a.d_cau_b
       : e < L.pb ? a.d_pair_w + (e - L.pw) : a.d_pair_b;
}

// dropout multipliers of rows r0 .. r0 + nr - 1, per row: emotion [D] | cause [D] | pair [2D].  The streams are indexed by the
// element of the whole batch, whichever rows a workgroup holds.
template <typename N>
__device__ __forceinline__ void fill_dropout_mults(const TailCore& a, float* mlt, int r0, int nr, int t, N nthr) {
  const int D = a.D, D2 = 2 * a.D, D4 = 4 * a.D;
  for (int e = t; e < nr * D4; e += nthr) {
    const int b = r0 + e / D4, k = e % D4;
    mlt[e] = k < D ? dropout_mult(a.d_emo, b * D + k) : (k < D2 ? dropout_mult(a.d_cau, b * D + (k - D)) : dropout_mult(a.d_pair, b * D2 + (k - D2)));
  }
}

// z = mu + eps * exp(log_var)   (sample_prior :345-351; std = exp(log_var))
__device__ __forceinline__ float reparam(float mu, float eps, float lv) { return mu + eps * expf(lv); }
// element k of [z_e | z_c] from one row of lat
__device__ __forceinline__ float sample_z(const float* row, const float* eps_e, const float* eps_c, int D, int k) {
  return (k < D) ? reparam(row[k], eps_e[k], row[D + k]) : reparam(row[2 * D + (k - D)], eps_c[k - D], row[3 * D + (k - D)]);
}

// logit h of local row b: h < EC emotion classes, EC cause, EC + 1 pair (0 beyond)
__device__ __forceinline__ float head_logit(const TailCore& a, const HeadLayout& L, const float* hw, const float* zl, const float* mlt, int b, int h) {
  const int D = a.D, D2 = 2 * a.D, D4 = 4 * a.D;
  float s = 0.f;
  if (h < a.EC) {
    s = hw[L.eb + h];
    for (int k = 0; k < D; ++k) s = fmaf(hw[h * D + k], zl[b * D2 + k] * mlt[b * D4 + k], s);
  } else if (h == a.EC) {
    s = hw[L.cb];
    for (int k = 0; k < D; ++k) s = fmaf(hw[L.cw + k], zl[b * D2 + D + k] * mlt[b * D4 + D + k], s);
  } else if (h == a.EC + 1) {
    s = hw[L.pb];
    for (int k = 0; k < D2; ++k) s = fmaf(hw[L.pw + k], zl[b * D2 + k] * mlt[b * D4 + D2 + k], s);
  }
  return s;
}

// pos_weight of the pair head from the batch's label sum (or the global batch's: the override, summed over the ranks in order)
__device__ __forceinline__ float pair_pos_weight(const TailCore& a, float ysum) {
  const float ntot = a.label_sum_override ? a.n_override : (float)a.B;
  float ytot = ysum;
  if (a.label_sum_override) {
    ytot = a.label_sum_override[0];
    for (int r = 1; r < a.label_sum_ranks; ++r) ytot += a.label_sum_override[(long)r * a.rank_stride];
  }
  return (ntot - ytot) / ytot;        // inf when there is no positive in the batch
}

// ---- row losses and dlogits.  lg: the row's 16 logits; bg: its index in the batch (labels); the dlogits carry weight / B.
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float smoothed(float y, float ls) { return y * (1.f - ls) + ls; }
// BCE on a probability as torch computes it (logs clamped at -100), and its derivative w.r.t. p
__device__ __forceinline__ float bce_prob(float p, float tg) { return -(tg * fmaxf(logf(p), -100.f) + (1.f - tg) * fmaxf(logf(1.f - p), -100.f)); }
__device__ __forceinline__ float bce_dprob(float p, float tg) { return (p - tg) / fmaxf((1.f - p) * p, 1e-12f); }
// sigmoid + BCE: d loss / d logit
__device__ __forceinline__ float sigmoid_bce_dlogit(float p, float tg) { const float gp = bce_dprob(p, tg); return gp * p * (1.f - p); }
// BCE-with-logits with pos_weight (lw = (pos_weight - 1) t + 1): loss and d loss / d logit
__device__ __forceinline__ float bce_logits_pw(float x, float tg, float lw) { return (1.f - tg) * x + lw * (log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.f)); }
__device__ __forceinline__ float bce_logits_pw_dlogit(float x, float tg, float lw) { return (1.f - tg) - lw * (1.f - sigmoidf(x)); }

// emotion: CE(W (z_e * m) + b, label), or the one-logit variant BCE(sigmoid(w (z_e * m) + b), smoothed label)
// (drl_classifier_ec_hsic.py:455-470).  LOSS: add the row's loss to l_emo; GRAD: write its dlogits to elog [8].  A kernel asks for
// what it needs: the single-workgroup one for both in one trip, the tiled phases for one each.
template <bool LOSS, bool GRAD>
__device__ __forceinline__ void emo_row(const TailCore& a, const float* lg, int bg, float& l_emo, float* elog) {
  if (!a.emo_bce) {
    float mx = -INFINITY;
    for (int c = 0; c < a.EC; ++c) mx = fmaxf(mx, lg[c]);
    float se = 0.f;
    for (int c = 0; c < a.EC; ++c) se += expf(lg[c] - mx);
    const float lse = mx + logf(se);
    long lab = a.emo_labels[bg]; lab = lab < 0 ? 0 : (lab >= a.EC ? a.EC - 1 : lab);
    if (LOSS) l_emo += lse - lg[lab];
    if (GRAD) for (int c = 0; c < a.EC; ++c) elog[c] = (expf(lg[c] - lse) - (c == lab ? 1.f : 0.f)) * (a.w_emo / a.B);
  } else {
    const float pe = sigmoidf(lg[0]);
    const float te = smoothed((float)a.emo_labels[bg], a.ls);
    if (LOSS) l_emo += bce_prob(pe, te);
    if (GRAD) elog[0] = sigmoid_bce_dlogit(pe, te) * (a.w_emo / a.B);
  }
}
// cause: BCE(sigmoid(w (z_c * m) + b), smoothed)
__device__ __forceinline__ float cau_row_loss(const TailCore& a, const float* lg, int bg) {
  return bce_prob(sigmoidf(lg[a.EC]), smoothed(a.cau_labels[bg], a.ls));
}
__device__ __forceinline__ float cau_row_dlogit(const TailCore& a, const float* lg, int bg) {
  return sigmoid_bce_dlogit(sigmoidf(lg[a.EC]), smoothed(a.cau_labels[bg], a.ls)) * (a.w_cau / a.B);
}
// pair: BCEWithLogits(w (z * m) + b, smoothed, pos_weight); dead = the batch-mean loss was infinite and is replaced by 0
__device__ __forceinline__ float pair_row_loss(const TailCore& a, const float* lg, int bg, float pw) {
  const float tp = smoothed(a.pair_labels[bg], a.ls);
  return bce_logits_pw(lg[a.EC + 1], tp, (pw - 1.f) * tp + 1.f);
}
__device__ __forceinline__ float pair_row_dlogit(const TailCore& a, const float* lg, int bg, float pw, bool dead) {
  const float tb = smoothed(a.pair_labels[bg], a.ls);
  return dead ? 0.f : bce_logits_pw_dlogit(lg[a.EC + 1], tb, (pw - 1.f) * tb + 1.f) * (a.w_pair / a.B);
}
// the three heads of one row, as the sums of tail_heads_kernel<1> take them ...
__device__ __forceinline__ void head_row_losses(const TailCore& a, const float* lg, int bg, float pw, float& l_emo, float& l_cau, float& l_pair) {
  emo_row<true, false>(a, lg, bg, l_emo, nullptr);
  l_cau += cau_row_loss(a, lg, bg);
  l_pair += pair_row_loss(a, lg, bg, pw);
}
// ... and their dlogits: elog [8] emotion, gx [2] cause / pair
__device__ __forceinline__ void head_row_dlogits(const TailCore& a, const float* lg, int bg, float pw, bool dead, float* elog, float* gx) {
  float unused = 0.f;
  emo_row<false, true>(a, lg, bg, unused, elog);
  gx[0] = cau_row_dlogit(a, lg, bg);
  gx[1] = pair_row_dlogit(a, lg, bg, pw, dead);
}

// ---- KL (:525-534) of element k of batch row b: the two sums, and its direct gradient on lat
__device__ __forceinline__ float kl_elem(float mu, float lv) { return -0.5f * (1.f + lv - expf(lv) - mu * mu); }
__device__ __forceinline__ void kl_row(const TailCore& a, int b, int k, float& kle, float& klc) {
  const int B = a.B, D = a.D;
  const float* row = a.lat + (long)b * 4 * D;
  const float mue = row[k], lve = row[D + k], muc = row[2 * D + k], lvc = row[3 * D + k];
  kle += kl_elem(mue, lve);
  klc += kl_elem(muc, lvc);
  float* dl = a.dlat_direct + (long)b * 4 * D;
  dl[k] = a.kl_w * mue / B; dl[D + k] = a.kl_w * (-0.5f) * (1.f - expf(lve)) / B;
  dl[2 * D + k] = a.kl_w * muc / B; dl[3 * D + k] = a.kl_w * (-0.5f) * (1.f - expf(lvc)) / B;
}

// ---- dz[b][k] from the three heads (local row b)
__device__ __forceinline__ float heads_dz(const TailCore& a, const HeadLayout& L, const float* hw, const float* mlt, const float* elog,
                                          const float* gx, int b, int k) {
  const int D = a.D, D2 = 2 * a.D, D4 = 4 * a.D;
  // The emotion or cause term is rounded on its own and the pair term is the fused one: the order both kernels had before the
  // formula moved here, named so that it does not hang on the compiler's choice of which product of a*b + c*d to contract
  // (it matters at dropout scales other than 1 and 2, where the products with mlt are inexact).
  float x;                                     // what reaches z[b][k] besides the pair head: the emotion classes (k < D) or the cause head
  if (k < D) {
    x = 0.f;
    for (int c = 0; c < a.EC; ++c) x = fmaf(hw[c * D + k], elog[b * 8 + c], x);
  } else {
    x = hw[L.cw + (k - D)] * gx[b * 2];
  }
  return fmaf(hw[L.pw + k] * gx[b * 2 + 1], mlt[b * D4 + D2 + k], __fmul_rn(x, mlt[b * D4 + k]));
}
// gradient of parameter element e of the image over local rows 0 .. nr - 1, in row order
__device__ __forceinline__ float head_param_grad(const TailCore& a, const HeadLayout& L, const float* zl, const float* mlt, const float* elog,
                                                 const float* gx, int e, int nr) {
  const int D = a.D, D2 = 2 * a.D, D4 = 4 * a.D;
  float s = 0.f;
  if (e < L.eb) {
    const int c = e / D, k = e - c * D;
    for (int b = 0; b < nr; ++b) s = fmaf(elog[b * 8 + c], zl[b * D2 + k] * mlt[b * D4 + k], s);
  } else if (e < L.cw) {
    const int c = e - L.eb;
    for (int b = 0; b < nr; ++b) s += elog[b * 8 + c];
  } else if (e < L.cb) {
    const int k = e - L.cw;
    for (int b = 0; b < nr; ++b) s = fmaf(gx[b * 2], zl[b * D2 + D + k] * mlt[b * D4 + D + k], s);
  } else if (e == L.cb) {
    for (int b = 0; b < nr; ++b) s += gx[b * 2];
  } else if (e < L.pb) {
    const int k = e - L.pw;
    for (int b = 0; b < nr; ++b) s = fmaf(gx[b * 2 + 1], zl[b * D2 + k] * mlt[b * D4 + D2 + k], s);
  } else {
    for (int b = 0; b < nr; ++b) s += gx[b * 2 + 1];
  }
  return s;
}

// ---- the MMD of nm samples per side from mmd_global_kernel's block partials: fixed order, double accumulation as in mmd_forward_block
__device__ __forceinline__ float mmd_from_partials(const TailCore& a, int nm) {
  double s11 = 0.0, s22 = 0.0, s12 = 0.0;
  for (int q = 0; q < a.mmd_nblk; ++q) { s11 += a.mmd_part[q * 4]; s22 += a.mmd_part[q * 4 + 1]; s12 += a.mmd_part[q * 4 + 2]; }
  const double b00 = 1.0 / ((double)nm * (nm - 1)), b01 = -1.0 / ((double)nm * nm);
  return (float)(2.0 * b01 * s12 + b00 * s11 + b00 * s22);
}
// terms[0..6] and pair_dead (one thread)
__device__ __forceinline__ void write_terms(const TailCore& a, float mmd, float dis_term, float l_emo, float l_cau, float l_pair, float kle,
                                            float klc, bool dead) {
  a.terms[1] = mmd; a.terms[2] = l_emo; a.terms[3] = l_cau; a.terms[4] = l_pair; a.terms[5] = kle; a.terms[6] = klc;
  a.terms[0] = dis_term + a.w_emo * l_emo + a.w_cau * l_cau + a.w_pair * l_pair + kle + klc;
  a.pair_dead[0] = dead ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------
// Decoder: logits[b][j] = z[b] . Wd[j] + bd[j] ; p = softmax_j ; rec = mean_{b,j} BCE(p, 0.9 bow + 0.1/V)
// Work is split over chunks of DEC_J vocabulary entries (one thread per entry holding its 2D weights in
// registers, latents in LDS).  Three passes (row max/sum, loss + softmax-backward dot, gradients); partial
// results are combined in fixed order so the result is run-to-run reproducible.
// decoder_kernel (whole batch in LDS) and decoder_tiled_kernel (batch tiles) keep their own pass loops; the per-element math is here.
// ------------------------------------------------------------------------------------------
constexpr int DEC_J = 128;          // vocabulary entries per workgroup
constexpr int DEC_MAXD2 = 64;
constexpr int DEC_MAXG = 4;         // sample groups per workgroup (threads = DEC_J * groups)

struct DecArgs {
  int B, D2, V;
  const float* z;          // [B, D2]
  const float* w; const float* b;          // [V, D2], [V]
  const float* bow;        // [B, V]
  float ls;
  float* part;             // pass1: [chunks][B][2] (max, sumexp) ; pass2: [chunks][B][2] (loss, dot)
  float* rowstat;          // [B][4]: M, log L, dot, loss-sum
  float* dz_part;          // [chunks][B][D2]
  float* dw; float* db;    // [V, D2], [V]
  float gscale;            // 1/(B V)
};

template <int CD2>
__device__ __forceinline__ float dec_logit(const float* wr, const float* zrow, int D2rt, float bias) {
  const int D2 = CD2 ? CD2 : D2rt;
  float s = bias;
  if (CD2 && (CD2 & 3) == 0) {
#pragma unroll
    for (int k = 0; k < D2; k += 4) {
      const float4 zv = *(const float4*)(zrow + k);          // LDS broadcast read, 16 B
      s = fmaf(wr[k], zv.x, s); s = fmaf(wr[k + 1], zv.y, s); s = fmaf(wr[k + 2], zv.z, s); s = fmaf(wr[k + 3], zv.w, s);
    }
  } else {
#pragma unroll
    for (int k = 0; k < D2; ++k) s = fmaf(wr[k], zrow[k], s);
  }
  return s;
}
__device__ __forceinline__ float dec_target(const DecArgs& a, float bow) { return bow * (1.f - a.ls) + a.ls / a.V; }
// element (b, j) from lp = its log softmax and tg = its target: the BCE and its term of the softmax-backward dot sum_j p_j dL/dp_j
__device__ __forceinline__ void dec_loss_dot(float lp, float tg, float& le, float& dt) {
  const float p = expf(lp);
  le = -(tg * fmaxf(lp, -100.f) + (1.f - tg) * fmaxf(log1pf(-p), -100.f));
  dt = p * bce_dprob(p, tg);
}

}  // namespace carel
