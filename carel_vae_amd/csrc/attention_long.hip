// Self-attention forward / backward for 128 < S <= 512 (multiples of 32), head_dim = 64: the flash-style counterpart of attention.hip,
// whose kernels hold one whole (sample, head) -- all of K and V -- in LDS and therefore stop at S = 128.  Reached through the same
// carel_attention_fwd / carel_attention_bwd entry points (attention.hip hands every S > 128 call to attn_long_fwd / attn_long_bwd);
// every S <= 128 call keeps its kernels.
//
// Forward  (attn_long_fwd_kernel): one workgroup = 4 waves = 128 queries of one (sample, head); each wave keeps its 32 queries' Q
//            fragments in registers and walks the key blocks (128 keys = four 32-key tiles, K and V staged as LDS images) with an
//            online softmax in the log2 domain: running max m and sum l per query, O rescaled by exp2(m_old - m_new) per block.
//            Layout as attention.hip: S^T = K Q^T with the KEY on the accumulator row and the QUERY on the lane, the probability tile
//            is directly the B operand of O^T = V^T P^T.
// Backward : two passes, no atomics (every gradient bitwise reproducible).
//   attn_long_dq_kernel   per 128-query block (the forward's layout): recomputes P from the saved lse, dP^T = V dO^T, and sums
//                         dQ^T = K^T dS^T over the key blocks; writes delta = rowsum(dO * O) of its queries to the workspace.
//   attn_long_dkv_kernel  per 128-key block (attention.hip's backward layout, key on the lane): walks the query blocks (Q, dO images,
//                         lse and delta in LDS) and sums dV^T = dO^T P and dK^T = Q^T dS; with the MPNet bias, each wave sums dS by
//                         distance into its own LDS array, the four are added in a fixed order and stored as one partial per
//                         (sample, head, key block); attn_long_drel_kernel adds a (sample, head)'s partials in key-block order to
//                         its row of d_rel_bias_dist.
// Bias by distance for S > 128: [12][1024], entry 511 + (key - query) (entry 1023 unused); its gradient [batch * 12][1024], same entry.
// The LDS image layout, its fragment readers, the kernel parameters and the softmax tile loop are attention_device.h's, shared with
// attention.hip.
#include "attention_device.h"

namespace carel {
namespace attn_long {

constexpr int SPAN = 1024;              // bias-by-distance row for S > 128
constexpr int ROFF = SPAN / 2 - 1;      // entry of distance 0

// -------------------------------------------------------------------------------------------------------- forward
template <bool REL, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_long_fwd_kernel(Params p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 16384 + 512 + (REL ? SPAN * 4 : 0)];
  char* kimg = smem;
  char* vimg = smem + 16384;
  float* maskadd = (float*)(smem + 32768);
  float* relb = (float*)(smem + 32768 + 512);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5;
  const int bh = blockIdx.x / p.nqb, qb = blockIdx.x - bh * p.nqb;
  const int b = bh / NH, h = bh - b * NH;
  const int S = p.S;
  long row0; int len;
  sample_rows(p, b, row0, len);
  const int nkt = (len + 31) >> 5;
  if (qb * 128 >= len) return;                       // whole workgroup: no query of this block exists
  const int q0 = qb * 128 + wave * 32;
  const bool qact = q0 < len && (p.qlim == 0 || q0 < p.qlim);      // wave-uniform
  const bf16_t* qbase = p.qkv + row0 * QKV_LD + h * HD;
  if (REL) for (int i = threadIdx.x; i < SPAN; i += 256) relb[i] = p.rel[h * SPAN + i];
  bf16x8 qf[4];
  if (qact) {
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = load_frag_global(qbase + (long)(q0 + (lane & 31)) * QKV_LD + 16 * s + 8 * hh);
  }
  const int q = q0 + (lane & 31);
  const uint32_t ebase = (uint32_t)((((long)b * NH + h) * S + q) * S) + (uint32_t)(4 * hh) + p.drop.idx_offset;
  f32x16 o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m = -INFINITY, lsum = 0.f;
  for (int kb = 0; kb * 4 < nkt; ++kb) {
    const int ktl = min(4, nkt - kb * 4);             // live key tiles of this block
    const int k0 = kb * 128;
    if (kb) __syncthreads();                          // every wave is done with the previous block's images
    stage_att(qbase + (long)k0 * QKV_LD + HID, QKV_LD, ktl * 32, kimg);
    stage_att(qbase + (long)k0 * QKV_LD + 2 * HID, QKV_LD, ktl * 32, vimg);
    int masked_here = 0;
    if (threadIdx.x < ktl * 32) {
      const int k = k0 + threadIdx.x;
      const float ma = p.cu ? (k < len ? 0.f : MASK_NEG) : ((p.att_mask && p.att_mask[row0 + k] == 0) ? MASK_NEG : 0.f);
      maskadd[threadIdx.x] = ma;
      masked_here = ma != 0.f;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int blk_masked = __syncthreads_or(masked_here);
    if (!qact) continue;
    f32x16 x[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) x[kt][r] = 0.f;
      if (kt < ktl) {
#pragma unroll
        for (int s = 0; s < 4; ++s) x[kt] = mfma32(frag32_row(kimg, kt * 32, s), qf[s], x[kt]);
      }
    }
    float mb = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      if (kt < ktl) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kl = kt * 32 + acc32_row(r, lane);
          float v = blk_masked ? fmaf(x[kt][r], SC2, maskadd[kl]) : x[kt][r] * SC2;
          if (REL) v = fmaf(relb[ROFF + k0 + kl - q], LOG2E, v);
          x[kt][r] = v;
          mb = fmaxf(mb, v);
        }
      }
    }
    mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
    const float mn = fmaxf(m, mb);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);      // 0 on the first block (m = -inf)
    m = mn;
    lsum *= alpha;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      if (kt < ktl) {
        exp2_dropout_tile<DROP>(x[kt], m, lsum, ebase + (uint32_t)(k0 + kt * 32), p.drop);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf16x8 pf = acc_as_operand(x[kt], s);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) o[dt] = mfma32(frag32_tr<true>(vimg, dt * 32, kt * 32 + 16 * s), pf, o[dt]);
        }
      }
    }
  }
  if (!qact) return;
  lsum += __shfl_xor(lsum, 32, 64);
  const bool qlive = q < len;
  if (hh == 0 && qlive) p.lse[((long)b * NH + h) * S + q] = (m + __builtin_amdgcn_logf(lsum)) * 0.6931471805599453f;
  const float inv = 1.0f / lsum;
  if (qlive) store_row_frags(o, inv, p.ctx + (row0 + q) * HID + h * HD, hh);
}

// -------------------------------------------------------------------------------------------------------- backward, dQ (+ delta)
// Per wave 32 queries on the lane, keys on the accumulator rows (the forward's layout).  Masked / past-the-sample keys get -inf through
// the mask term (probability exactly 0); a fully masked row's lse (-3.4e38) is clamped finite as in attention.hip.
template <bool REL, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_long_dq_kernel(Params p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 16384 + 512 + (REL ? SPAN * 4 : 0)];
  char* kimg = smem;
  char* vimg = smem + 16384;
  float* madd = (float*)(smem + 32768);
  float* relb = (float*)(smem + 32768 + 512);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5;
  const int bh = blockIdx.x / p.nqb, qb = blockIdx.x - bh * p.nqb;
  const int b = bh / NH, h = bh - b * NH;
  const int S = p.S;
  long row0; int len;
  sample_rows(p, b, row0, len);
  const int nkt = (len + 31) >> 5;
  if (qb * 128 >= len) return;
  const int q0 = qb * 128 + wave * 32;
  const int q = q0 + (lane & 31);
  const bool qexist = q0 < len;
  const bool qact = qexist && (p.qlim == 0 || q0 < p.qlim);       // wave-uniform; queries past q_rows: dQ = 0
  const bf16_t* qbase = p.qkv + row0 * QKV_LD + h * HD;
  bf16_t* out = p.dqkv + (row0 + q0) * QKV_LD + h * HD;
  if (qexist && !qact) {          // rows past q_rows: zero dQ (rows of the sample only); lane = (row, half of the 64 d)
    const int row = lane >> 1, half = lane & 1;
    if (q0 + row < len) {
      uint4* d = (uint4*)(out + (long)row * QKV_LD + half * 32);
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  if (p.qlim && qb * 128 >= p.qlim) return;       // whole workgroup past q_rows: nothing but the zeros above
  if (REL) for (int i = threadIdx.x; i < SPAN; i += 256) relb[i] = p.rel[h * SPAN + i];
  bf16x8 qf[4], dof[4];
  float lse2 = 0.f, dl = 0.f;
  if (qact) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long r = (long)(q0 + (lane & 31));
      qf[j] = load_frag_global(qbase + r * QKV_LD + 16 * j + 8 * hh);
      dof[j] = load_frag_global(p.dctx + (row0 + r) * HID + h * HD + 16 * j + 8 * hh);
      const bf16x8 of = load_frag_global(p.ctx + (row0 + r) * HID + h * HD + 16 * j + 8 * hh);
      const s16x8 a = __builtin_bit_cast(s16x8, dof[j]), c = __builtin_bit_cast(s16x8, of);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += bf2f((bf16_t)a[e]) * bf2f((bf16_t)c[e]);
    }
    s += __shfl_xor(s, 32, 64);
    dl = q < len ? s : 0.f;
    if (hh == 0 && q < len) p.delta[(long)bh * S + q] = dl;
    lse2 = q < len ? fmaxf(p.lse[(long)bh * S + q], -1e30f) * LOG2E : INFINITY;
  }
  const uint32_t ebase = (uint32_t)((((long)b * NH + h) * S + q) * S) + (uint32_t)(4 * hh) + p.drop.idx_offset;
  f32x16 dq[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
  for (int kb = 0; kb * 4 < nkt; ++kb) {
    const int ktl = min(4, nkt - kb * 4);
    const int k0 = kb * 128;
    if (kb) __syncthreads();
    stage_att(qbase + (long)k0 * QKV_LD + HID, QKV_LD, ktl * 32, kimg);
    stage_att(qbase + (long)k0 * QKV_LD + 2 * HID, QKV_LD, ktl * 32, vimg);
    if (threadIdx.x < ktl * 32) {
      const int k = k0 + threadIdx.x;
      const bool masked = p.cu ? k >= len : (p.att_mask && p.att_mask[row0 + k] == 0);
      madd[threadIdx.x] = masked ? -INFINITY : 0.f;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!qact) continue;
    for (int kt = 0; kt < ktl; ++kt) {
      f32x16 sa, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sa[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sa = mfma32(frag32_row(kimg, kt * 32, s), qf[s], sa);      // S^T[k][q]
        dp = mfma32(frag32_row(vimg, kt * 32, s), dof[s], dp);     // dP^T[k][q]
      }
      f32x16 dsv;
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        float dm0 = 1.0f, dm1 = 1.0f;
        if constexpr (DROP) {
          const uint32_t hsh = mix32(((ebase + (uint32_t)(k0 + kt * 32 + (r & 3) + 8 * (r >> 2))) >> 1) ^ p.drop.key);
          dm0 = dropout_pick(p.drop, hsh, 0u); dm1 = dropout_pick(p.drop, hsh, 1u);
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int kl = kt * 32 + acc32_row(r + e, lane);
          float arg = fmaf(sa[r + e], SC2, madd[kl] - lse2);
          if (REL) arg = fmaf(relb[ROFF + k0 + kl - q], LOG2E, arg);
          const float pr = __builtin_amdgcn_exp2f(arg);
          dsv[r + e] = pr * fmaf(dp[r + e], e ? dm1 : dm0, -dl);
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 df = acc_as_operand(dsv, s);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) dq[dt] = mfma32(frag32_tr<true>(kimg, dt * 32, kt * 32 + 16 * s), df, dq[dt]);
      }
    }
  }
  if (!qact) return;
  if (q < len) store_row_frags(dq, 0.125f, out + (long)(lane & 31) * QKV_LD, hh);
}

// -------------------------------------------------------------------------------------------------------- backward, dK / dV
constexpr int DKV_LDS = 16384 + 16384 + 1024;
constexpr int DKV_LDS_REL = DKV_LDS + SPAN * 4 + 4 * SPAN * 4;
template <bool REL, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_long_dkv_kernel(Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // DKV_LDS (REL: DKV_LDS_REL) bytes
  char* qimg = smem;
  char* doimg = smem + 16384;
  float* lse = (float*)(smem + 32768);
  float* delta = lse + 128;
  float* relb = (float*)(smem + DKV_LDS);           // REL: bias by distance [1024], then the waves' gradient sums [4][1024]
  float* relg = relb + SPAN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5;
  const int bh = blockIdx.x / p.nkb, kb = blockIdx.x - bh * p.nkb;
  const int b = bh / NH, h = bh - b * NH;
  const int S = p.S;
  long row0; int len;
  sample_rows(p, b, row0, len);
  const int nt = (len + 31) >> 5, rows = nt << 5;
  if (kb * 128 >= rows) return;
  const int ntq = p.qlim ? min(nt, p.qlim >> 5) : nt;
  const bf16_t* qbase = p.qkv + row0 * QKV_LD + h * HD;
  const bf16_t* dobase = p.dctx + row0 * HID + h * HD;
  if (REL) {
    for (int i = threadIdx.x; i < SPAN; i += 256) relb[i] = p.rel[h * SPAN + i];
    for (int i = threadIdx.x; i < 4 * SPAN; i += 256) relg[i] = 0.f;
  }
  const int kw = kb * 128 + wave * 32;
  const bool active = kw < rows;
  const int key = kw + (lane & 31);
  bf16x8 kf[4], vf[4];
  float madd2 = -INFINITY;
  if (active) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      kf[s] = load_frag_global(qbase + HID + (long)key * QKV_LD + 16 * s + 8 * hh);
      vf[s] = load_frag_global(qbase + 2 * HID + (long)key * QKV_LD + 16 * s + 8 * hh);
    }
    const bool klive = key < len;
    madd2 = p.cu ? (klive ? 0.f : -INFINITY) : ((p.att_mask && p.att_mask[row0 + key] == 0) ? -INFINITY : 0.f);
  }
  const uint32_t hbase = (uint32_t)(((long)b * NH + h) * S * S) + (uint32_t)(key & ~1) + (uint32_t)((16 * (lane & 1) + 4 * hh) * S) + p.drop.idx_offset;
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[dt][r] = 0.f; dv[dt][r] = 0.f; }
  for (int qb = 0; qb * 4 < ntq; ++qb) {
    const int qtl = min(4, ntq - qb * 4);
    const int qs0 = qb * 128;
    if (qb) __syncthreads();
    stage_att(qbase + (long)qs0 * QKV_LD, QKV_LD, qtl * 32, qimg);
    stage_att(dobase + (long)qs0 * HID, HID, qtl * 32, doimg);
    if (threadIdx.x < 128) {
      const int qq = qs0 + threadIdx.x;
      const bool live = qq < len && threadIdx.x < qtl * 32;
      lse[threadIdx.x] = live ? fmaxf(p.lse[(long)bh * S + qq], -1e30f) * LOG2E : INFINITY;
      delta[threadIdx.x] = live ? p.delta[(long)bh * S + qq] : 0.f;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) continue;
    for (int qt = 0; qt < qtl; ++qt) {
      const int qg = qs0 + qt * 32;                  // first query of the tile
      f32x16 sa, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sa[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sa = mfma32(frag32_row(qimg, qt * 32, s), kf[s], sa);     // S[q][k]
        dp = mfma32(frag32_row(doimg, qt * 32, s), vf[s], dp);    // dP[q][k]
      }
      uint32_t hown[8], hoth[8];
      const uint32_t odd = (uint32_t)lane & 1u;
      if constexpr (DROP) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          hown[j] = mix32(((hbase + (uint32_t)((qg + (j & 3) + 8 * (j >> 2)) * S)) >> 1) ^ p.drop.key);
          hoth[j] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hown[j], 0xB1, 0xF, 0xF, true);
        }
      }
      f32x16 pd, dsv;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 l4 = *(const f32x4*)(lse + qt * 32 + 8 * i + 4 * hh);
        const f32x4 d4 = *(const f32x4*)(delta + qt * 32 + 8 * i + 4 * hh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * i + e;
          float arg = fmaf(sa[r], SC2, madd2 - l4[e]);
          if (REL) arg = fmaf(relb[ROFF + key - (qg + 8 * i + 4 * hh + e)], LOG2E, arg);
          const float pr = __builtin_amdgcn_exp2f(arg);
          float dm = 1.0f;
          if constexpr (DROP) dm = dropout_pick(p.drop, ((uint32_t)(r >> 3) == odd) ? hown[r & 7] : hoth[r & 7], odd);
          pd[r] = pr * dm;
          dsv[r] = pr * fmaf(dp[r], dm, -d4[e]);
        }
      }
      if (REL) {      // each wave into its own array; the two half-waves (same keys, queries 4 apart) take turns: no shared address per instruction
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float* mine = relg + wave * SPAN + ROFF + key - (qg + acc32_row(r, lane));
          if (hh == 0) *mine += dsv[r];
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (hh == 1) *mine += dsv[r];
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pf = acc_as_operand(pd, s), df = acc_as_operand(dsv, s);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt] = mfma32(frag32_tr<true>(doimg, dt * 32, qt * 32 + 16 * s), pf, dv[dt]);   // dV^T[d][k]
          dk[dt] = mfma32(frag32_tr<true>(qimg, dt * 32, qt * 32 + 16 * s), df, dk[dt]);    // dK^T[d][k]
        }
      }
    }
  }
  __syncthreads();                       // every wave is done with the images and its bias sums
  if (REL) {
    float* part = p.drel_part + ((long)bh * p.nkb + kb) * SPAN;
    for (int i = threadIdx.x; i < SPAN; i += 256) part[i] = ((relg[i] + relg[SPAN + i]) + relg[2 * SPAN + i]) + relg[3 * SPAN + i];
  }
  if (!active) return;
  char* slot = qimg + wave * 4096;
  bf16_t* out = p.dqkv + (row0 + kw) * QKV_LD + h * HD;
  store_rows_via_lds(dk, 0.125f, slot, out + HID, QKV_LD, kw, len);
  store_rows_via_lds(dv, 1.0f, slot, out + 2 * HID, QKV_LD, kw, len);
}

// d_rel_bias_dist row (sample, head) += its key blocks' partials, in key-block order (no atomics)
__global__ __launch_bounds__(256) void attn_long_drel_kernel(Params p) {
  const int bh = blockIdx.x, b = bh / NH;
  long row0; int len;
  sample_rows(p, b, row0, len);
  const int nkb = (((len + 31) >> 5) + 3) >> 2;
  for (int i = threadIdx.x; i < SPAN; i += 256) {
    float s = 0.f;
    for (int kb = 0; kb < nkb; ++kb) s += p.drel_part[((long)bh * p.nkb + kb) * SPAN + i];
    p.drel[(long)bh * SPAN + i] += s;
  }
}

// ------------------------------------------------------------------------------------------------ MPNet relative positions, span 256 / 1024
// dist [NH][span]: entry i = table[bucket[i]][h] (distance i - (span/2 - 1); entry span - 1 unused, written 0)
__global__ void relpos_expand_span_kernel(const float* table, const int* bucket, float* dist, int span) {
  const int h = blockIdx.x;
  for (int i = threadIdx.x; i < span; i += 256) dist[h * span + i] = i < span - 1 ? table[bucket[i] * NH + h] : 0.f;
}
// ddist [batch * NH][span] -> dtable [32][NH]: samples in order, then distances in order (span 256: the bits of carel_relpos_reduce)
__global__ __launch_bounds__(256) void relpos_reduce_span_kernel(const float* ddist, int batch, const int* bucket, float* dtable, int accumulate, int span) {
  __shared__ float bydist[SPAN];
  const int h = blockIdx.x;
  for (int i = threadIdx.x; i < span; i += 256) {
    float s = 0.f;
    for (int b = 0; b < batch; ++b) s += ddist[((long)b * NH + h) * span + i];
    bydist[i] = s;
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i < 32) {
    float t = 0.f;
    for (int d = 0; d < span - 1; ++d) if (bucket[d] == i) t += bydist[d];
    dtable[i * NH + h] = accumulate ? dtable[i * NH + h] + t : t;
  }
}

}  // namespace attn_long
}  // namespace carel

using namespace carel;
using namespace carel::attn_long;

namespace {
size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
int n_blocks(int S) { return (S + 127) / 128; }
size_t delta_bytes(long B, int S) { return al256((size_t)B * NH * S * 4); }
}  // namespace

extern "C" int64_t carel_attention_bwd_workspace_bytes(int32_t batch, int32_t seq_len, int32_t with_rel) {
  if (batch < 1 || seq_len <= 128) return 0;
  size_t n = delta_bytes(batch, seq_len);
  if (with_rel) n += al256((size_t)batch * NH * n_blocks(seq_len) * SPAN * 4);
  return (int64_t)n;
}

namespace carel {
// Called by attention.hip for seq_len > 128 with the parameters attn_prepare has checked and filled; what is added here is the grid's
// block counts and, in the backward, the workspace's two arrays.
static Params long_params(const AttnParams& q) {
  Params p;
  static_cast<AttnCommon&>(p) = q;
  p.drel = q.drel;
  p.nqb = n_blocks(p.S); p.nkb = p.nqb;
  if (p.qlim) p.nqb = n_blocks(p.qlim);
  p.delta = nullptr; p.drel_part = nullptr;
  return p;
}

int attn_long_fwd(const AttnParams& q, hipStream_t stream) {
  const Params p = long_params(q);
  ATTN_LAUNCH(attn_long_fwd_kernel, dim3(p.B * NH * p.nqb), 0, 0, stream, p);
  return check_launch("attn_long_fwd_kernel");
}

int attn_long_bwd(const AttnParams& q, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  Params p = long_params(q);
  const int64_t need = carel_attention_bwd_workspace_bytes(p.B, p.S, p.rel ? 1 : 0);
  if (!workspace || workspace_bytes < need)
    return set_error(CAREL_ERR_ARG, "%s: seq_len %d needs a workspace of carel_attention_bwd_workspace_bytes() = %lld bytes (got %lld)",
                     "carel_attention_bwd", p.S, (long long)need, (long long)workspace_bytes);
  p.delta = (float*)workspace;
  if (p.rel) p.drel_part = (float*)((char*)workspace + delta_bytes(p.B, p.S));
  p.nqb = p.nkb;                    // the dQ pass covers every query block: rows past q_rows get their zeros there
  ATTN_DYNAMIC_LDS(attn_long_dkv_kernel, DKV_LDS, DKV_LDS_REL);
  int rc;
  const dim3 grid(p.B * NH * p.nkb);
  ATTN_LAUNCH(attn_long_dq_kernel, grid, 0, 0, stream, p);
  if ((rc = check_launch("attn_long_dq_kernel"))) return rc;
  ATTN_LAUNCH(attn_long_dkv_kernel, grid, DKV_LDS, DKV_LDS_REL, stream, p);
  if ((rc = check_launch("attn_long_dkv_kernel"))) return rc;
  if (p.rel) {
    hipLaunchKernelGGL(attn_long_drel_kernel, dim3(p.B * NH), dim3(256), 0, stream, p);
    if ((rc = check_launch("attn_long_drel_kernel"))) return rc;
  }
  return CAREL_OK;
}
}  // namespace carel

// The learned table is relative_attention_bias.weight [32 buckets][12 heads]; bucket[i] (int32 [span], entry i = distance key - query
// = i - (span/2 - 1), the last entry unused) is computed by the caller with the very expression of transformers
// MPNetEncoder.relative_position_bucket (a float32 log and a truncation: not re-derived here, so no rounding can differ).
extern "C" int carel_relpos_expand_span(const void* table, const void* bucket, void* dist, int32_t span, void* stream) {
  if (!table || !bucket || !dist) return set_error(CAREL_ERR_ARG, "carel_relpos_expand_span: null tensor");
  if (span != 256 && span != SPAN) return set_error(CAREL_ERR_ARG, "carel_relpos_expand_span: span must be 256 or 1024 (got %d)", span);
  hipLaunchKernelGGL(relpos_expand_span_kernel, dim3(NH), dim3(256), 0, (hipStream_t)stream, (const float*)table, (const int*)bucket, (float*)dist, (int)span);
  return check_launch("relpos_expand_span_kernel");
}
extern "C" int carel_relpos_reduce_span(const void* ddist, int32_t batch, const void* bucket, void* dtable, int32_t accumulate, int32_t span, void* stream) {
  if (!ddist || !bucket || !dtable || batch < 1) return set_error(CAREL_ERR_ARG, "carel_relpos_reduce_span: null tensor or batch < 1");
  if (span != 256 && span != SPAN) return set_error(CAREL_ERR_ARG, "carel_relpos_reduce_span: span must be 256 or 1024 (got %d)", span);
  hipLaunchKernelGGL(relpos_reduce_span_kernel, dim3(NH), dim3(256), 0, (hipStream_t)stream, (const float*)ddist, (int)batch, (const int*)bucket,
                     (float*)dtable, (int)accumulate, (int)span);
  return check_launch("relpos_reduce_span_kernel");
}
// the span-256 forms (S <= 128), as they were before there was a second span
extern "C" int carel_relpos_expand(const void* table, const void* bucket, void* dist, void* stream) {
  if (!table || !bucket || !dist) return set_error(CAREL_ERR_ARG, "carel_relpos_expand: null tensor");
  return carel_relpos_expand_span(table, bucket, dist, 256, stream);
}
extern "C" int carel_relpos_reduce(const void* ddist, int32_t batch, const void* bucket, void* dtable, int32_t accumulate, void* stream) {
  if (!ddist || !bucket || !dtable || batch < 1) return set_error(CAREL_ERR_ARG, "carel_relpos_reduce: null tensor or batch < 1");
  return carel_relpos_reduce_span(ddist, batch, bucket, dtable, accumulate, 256, stream);
}
