// Adversarial (GAN) disentangler of the two-space ablation script drl_classifier_ec_gan.py: the two one-logit adversaries
//   ec_disc: sigmoid(w . dropout(c.detach()) + b) against the emotion labels   (:222-225, :430-442)
//   ce_disc: sigmoid(w . dropout(e.detach()) + b) against the cause labels     (:231-234, :444-456)
// their BCE losses on smoothed labels (:458-470) and the entropy terms mean_b p log(p + epsilon) (:472-477) that the vae loss adds.
// z = [e | c] f32 [B, 2D], D <= 32, B <= 1024.  One workgroup of 512 threads:
//   phase 1  thread per sample: both logits, the four per-sample loss summands (block sums, fixed order) and the four gradients at
//            the logit, kept in LDS;
//   phase 2  thread per (discriminator, column, batch quarter): both gradient images of that column over the samples of the quarter
//            in ascending order (the dropout multiplier is recomputed from the hash), then the four quarters are added in order.
// No atomics: the same inputs give the same bits.  Nothing reaches z (the embeddings are detached): there is no dz.
#include "carel_hip_internal.h"

namespace carel {

constexpr int GAN_THREADS = 512, GAN_COLS = 128, GAN_PARTS = GAN_THREADS / GAN_COLS, GAN_MAX_B = 1024;

struct GanArgs {
  const float* z; int B, D;
  const float* y[2];            // labels of disc 0 (emotion), disc 1 (cause)
  const float* w[2]; const float* b[2];
  float ls, eps, w_ent;
  Dropout drop[2];
  const float* vae_in;
  float* terms;
  float* g_loss_w[2]; float* g_loss_b[2]; float* g_ent_w[2]; float* g_ent_b[2];
};

// input of discriminator d for sample b: ec_disc reads the cause half of z, ce_disc the emotion half
__device__ __forceinline__ float gan_x(const GanArgs& a, int d, int b, int k) {
  const float v = a.z[(long)b * 2 * a.D + (d == 0 ? a.D : 0) + k];
  return v * dropout_mult(a.drop[d], (uint32_t)(b * a.D + k));
}

__global__ __launch_bounds__(GAN_THREADS) void gan_disc_kernel(GanArgs a) {
  __shared__ float red[16];
  __shared__ float dl[2][2][GAN_MAX_B];                 // [disc][0 loss, 1 entropy][sample]: gradient at the logit, 1/B included
  __shared__ float part[GAN_PARTS][GAN_COLS][2];
  const int B = a.B, D = a.D, t = threadIdx.x;
  const float invB = 1.0f / (float)B;
  float s_loss[2] = {0.f, 0.f}, s_ent[2] = {0.f, 0.f};
  for (int b = t; b < B; b += GAN_THREADS) {
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      float x = a.b[d][0];
      for (int k = 0; k < D; ++k) x = fmaf(a.w[d][k], gan_x(a, d, b, k), x);
      const float p = 1.0f / (1.0f + expf(-x)), q = 1.0f / (1.0f + expf(x));      // q = 1 - p without the cancellation
      const float tgt = a.y[d][b] * (1.f - a.ls) + a.ls;                            // ec_num_class = 1 (:466)
      s_loss[d] += -(tgt * fmaxf(logf(p), -100.f) + (1.f - tgt) * fmaxf(logf(q), -100.f));
      const float lpe = logf(p + a.eps);
      s_ent[d] += p * lpe;
      const float pq = p * q;
      dl[d][0][b] = (p - tgt) / fmaxf(pq, 1e-12f) * pq * invB;                      // BCELoss backward (its 1e-12 clamp), then sigmoid'
      dl[d][1][b] = (lpe + p / (p + a.eps)) * pq * invB;
    }
  }
  float tot[4];
  tot[0] = block_sum(s_loss[0], red) * invB;
  tot[1] = block_sum(s_loss[1], red) * invB;
  tot[2] = block_sum(s_ent[0], red) * invB;
  tot[3] = block_sum(s_ent[1], red) * invB;            // (the barriers of block_sum also publish dl)
  if (t == 0) {
    for (int i = 0; i < 4; ++i) a.terms[i] = tot[i];
    if (a.vae_in) a.terms[4] = a.vae_in[0] + a.w_ent * (tot[2] + tot[3]);
  }
  // gradient images: column k < D = weight k, column D = bias
  const int col = t & (GAN_COLS - 1), pt = t / GAN_COLS;
  const int d = col / (D + 1), k = col - d * (D + 1);
  float gl = 0.f, ge = 0.f;
  if (d < 2) {
    for (int b = pt; b < B; b += GAN_PARTS) {
      const float x = k < D ? gan_x(a, d, b, k) : 1.0f;
      gl = fmaf(dl[d][0][b], x, gl);
      ge = fmaf(dl[d][1][b], x, ge);
    }
  }
  part[pt][col][0] = gl; part[pt][col][1] = ge;
  __syncthreads();
  if (pt == 0 && d < 2) {
    float l = part[0][col][0], e = part[0][col][1];
#pragma unroll
    for (int p = 1; p < GAN_PARTS; ++p) { l += part[p][col][0]; e += part[p][col][1]; }
    if (k < D) { a.g_loss_w[d][k] = l; a.g_ent_w[d][k] = e; }
    else { a.g_loss_b[d][0] = l; a.g_ent_b[d][0] = e; }
  }
}

}  // namespace carel

using namespace carel;

extern "C" int carel_gan_disc(const carel_gan_args* a, void* stream) {
  const char* who = "carel_gan_disc";
  if (!a) return set_error(CAREL_ERR_ARG, "%s: null arguments", who);
  if (!a->z || !a->emo_labels || !a->cau_labels || !a->terms) return set_error(CAREL_ERR_ARG, "%s: null tensor", who);
  for (int i = 0; i < 2; ++i)
    if (!a->disc_w[i] || !a->disc_b[i] || !a->g_loss_w[i] || !a->g_loss_b[i] || !a->g_ent_w[i] || !a->g_ent_b[i])
      return set_error(CAREL_ERR_ARG, "%s: null discriminator tensor", who);
  if (a->batch < 1 || a->batch > GAN_MAX_B || a->ec_dim < 1 || a->ec_dim > 32)
    return set_error(CAREL_ERR_SHAPE, "%s: need 1 <= batch <= %d and 1 <= ec_dim <= 32; got batch %d, ec_dim %d", who, GAN_MAX_B, a->batch, a->ec_dim);
  if (!(a->drop_p >= 0.f && a->drop_p <= 1.f) || !(a->label_smoothing >= 0.f && a->label_smoothing <= 1.f) || !(a->epsilon >= 0.f))
    return set_error(CAREL_ERR_ARG, "%s: drop_p and label_smoothing must lie in [0, 1], epsilon must not be negative", who);
  static_assert(2 * (32 + 1) <= GAN_COLS, "one thread per (discriminator, column)");
  GanArgs k;
  k.z = (const float*)a->z; k.B = a->batch; k.D = a->ec_dim;
  k.y[0] = (const float*)a->emo_labels; k.y[1] = (const float*)a->cau_labels;
  for (int i = 0; i < 2; ++i) {
    k.w[i] = (const float*)a->disc_w[i]; k.b[i] = (const float*)a->disc_b[i];
    k.g_loss_w[i] = (float*)a->g_loss_w[i]; k.g_loss_b[i] = (float*)a->g_loss_b[i];
    k.g_ent_w[i] = (float*)a->g_ent_w[i]; k.g_ent_b[i] = (float*)a->g_ent_b[i];
    k.drop[i] = make_dropout(a->drop_seed, 103u + (uint32_t)i, a->drop_p, a->drop_row_offset * (uint32_t)a->ec_dim);
  }
  k.ls = a->label_smoothing; k.eps = a->epsilon; k.w_ent = a->w_entropy;
  k.vae_in = (const float*)a->vae_loss_in; k.terms = (float*)a->terms;
  hipLaunchKernelGGL(gan_disc_kernel, dim3(1), dim3(GAN_THREADS), 0, (hipStream_t)stream, k);
  return check_launch("gan_disc_kernel");
}
