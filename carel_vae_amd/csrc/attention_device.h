// What the two attention kernel families share -- attention.hip (S <= 128: one whole (sample, head) in LDS) and attention_long.hip
// (128 < S <= 512: flash-style blocks of 128) -- so that both read the same LDS images with the same swizzle, pair their dropout
// hashes the same way and take the same arguments: the constants, the image layout and its fragment readers, the kernel parameter
// structs and the REL x DROP launch helper.
#pragma once
#include "carel_hip_internal.h"

namespace carel {

constexpr int HD = 64;        // head dim
constexpr int NH = 12;        // heads
constexpr int HID = NH * HD;  // 768
constexpr int QKV_LD = 3 * HID;
constexpr float MASK_NEG = -3.4028234663852886e38f;   // torch.finfo(float32).min, as HF adds it
constexpr float LOG2E = 1.4426950408889634f;
constexpr float SC2 = 0.125f * LOG2E;                 // 1/sqrt(head dim) and log2(e) in one multiply: the scores live in the log2 domain

// K/V/Q/dO tiles are LDS images with 128-B rows filled by global_load_lds_dwordx4; the XOR swizzle f_att serves both the row reads
// (ds_read_b128) and the transposed reads (ds_read_b64_tr_b16).
__device__ __forceinline__ int f_att(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ int att_off(int row, int chunk) { return row * 128 + ((chunk ^ f_att(row)) << 4); }

// fill an image of `rows` x 64 bf16 (rows a multiple of 8, <= 128) from a row-major global matrix (row stride ld elements); 256 threads
__device__ __forceinline__ void stage_att(const bf16_t* __restrict__ g, long ld, int rows, char* img) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int q = wave; q < (rows >> 3); q += 4) {
    const int r = q * 8 + (lane >> 3);
    const int c = (lane & 7) ^ f_att(r);
    __builtin_amdgcn_global_load_lds(g + (long)r * ld + c * 8, (CAREL_LDS void*)(img + q * 1024), 16, 0, 0);
  }
}

// 32x32x16 operand whose own-matrix row is on the lane: X[row = r0 + (l&31)][kk = 16*s + 8*(l>>5) + j]
__device__ __forceinline__ bf16x8 frag32_row(const char* img, int r0, int s) {
  const int l = threadIdx.x & 63;
  return *(const bf16x8*)(img + att_off(r0 + (l & 31), 2 * s + (l >> 5)));
}
// 32x32x16 operand read TRANSPOSED from an image M[kk][x]: lane holds M[kk(j)][x = x0 + (l&31)].
//   PERM = false: kk(j) = kb + 8*(l>>5) + j                      (natural order)
//   PERM = true : kk(j) = kb + 8*(j>>2) + 4*(l>>5) + (j&3)        (pairs with an accumulator tile used as
//                                                                  the other operand, carel_common.h)
template <bool PERM>
__device__ __forceinline__ bf16x8 frag32_tr(const char* img, int x0, int kb) {
  const int l = threadIdx.x & 63;
  const int g = l >> 4, hh = g >> 1, qq = (l & 15) >> 2, p = l & 3;
  const int chunk = ((x0 + 16 * (g & 1)) >> 3) + (p >> 1), sub = (p & 1) * 8;
  const int r0 = PERM ? (kb + 4 * hh + qq) : (kb + 8 * hh + qq);
  const int r1 = PERM ? (r0 + 8) : (r0 + 4);
  s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((CAREL_LDS s16x4*)(img + att_off(r0, chunk) + sub));
  s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((CAREL_LDS s16x4*)(img + att_off(r1, chunk) + sub));
  s16x8 r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// registers 8s..8s+7 of a 32x32 accumulator as the bf16 B operand of k-step s (rows of the tile = kk)
__device__ __forceinline__ bf16x8 acc_as_operand(const f32x16& x, int s) {
  const uint4 r = {pack2bf(x[8 * s], x[8 * s + 1]), pack2bf(x[8 * s + 2], x[8 * s + 3]), pack2bf(x[8 * s + 4], x[8 * s + 5]), pack2bf(x[8 * s + 6], x[8 * s + 7])};
  return __builtin_bit_cast(bf16x8, r);
}

__device__ __forceinline__ bf16x8 load_frag_global(const bf16_t* p) { return *(const bf16x8*)p; }

// A wave's [32 rows][64 d] result sits in two 32x32 accumulators with the ROW on the lane and 4-element groups of d spread over
// the registers and the two half-waves: stored straight from there every instruction writes 16-byte fragments of 32 different
// rows (8 instructions per 128-byte line; measured: the stores were 27 % of the backward kernel).  Through a 4-KiB LDS slot of the
// wave's own (XOR-swizzled 16-byte chunks: conflict-free both ways) every instruction stores 8 whole 128-byte rows instead.
__device__ __forceinline__ void store_rows_via_lds(const f32x16 (&acc)[2], float scale, char* slot, bf16_t* grow0, long ld, int row_base, int nrows_live) {
  const int l = threadIdx.x & 63, r = l & 31, hh = l >> 5;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = dt * 32 + 8 * i + 4 * hh;                          // 4 consecutive d
      const int chunk = (d >> 3) ^ ((r >> 1) & 7);
      const uint2 v = {pack2bf(acc[dt][4 * i] * scale, acc[dt][4 * i + 1] * scale), pack2bf(acc[dt][4 * i + 2] * scale, acc[dt][4 * i + 3] * scale)};
      *(uint2*)(slot + r * 128 + chunk * 16 + (d & 4) * 2) = v;
    }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                   // the slot is this wave's own: no barrier needed
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = it * 8 + (l >> 3), c = l & 7;
    const uint4 v = *(const uint4*)(slot + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
    if (row_base + row < nrows_live) *(uint4*)(grow0 + (long)row * ld + c * 8) = v;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                   // reads done before the slot is rewritten
}

// ------------------------------------------------------------------------------------------------ kernel parameters
// what every attention kernel takes; attn_prepare (attention.hip) checks the call and fills it
struct AttnCommon {
  const bf16_t* qkv;        // [B*S, 2304]
  const long* att_mask;     // [B, S] (1 = attend) or null
  bf16_t* ctx;              // fwd out / bwd in  [B*S, 768]
  float* lse;               // [B, NH, S]
  const bf16_t* dctx;       // bwd in   [B*S, 768]
  bf16_t* dqkv;             // bwd out  [B*S, 2304]
  int B, S;
  Dropout drop;             // element index ((b*NH + h)*S + q)*S + k
  const int* cu;            // packed: rows [cu[b], cu[b+1]) belong to sample b (null = dense, rows b*S ..)
  const float* rel;         // MPNet relative-position bias by distance: [NH][256], entry 127 + (key - query), for S <= 128;
                            // [NH][1024], entry 511 + (key - query), for S > 128; null = none
  int qlim;                 // 0 = all; else only the first qlim (multiple of 32) positions of every sample are live queries
};
struct AttnParams : AttnCommon {      // S <= 128
  float* drel;              // bwd: its gradient by distance, [B * NH][256]: row (sample, head) is read-modify-written by that workgroup alone (every
                            // layer adds to it in stream order) -- no atomics anywhere, so the table gradient is bit-reproducible
};
namespace attn_long {
struct Params : AttnCommon {          // S > 128
  float* delta;             // bwd workspace: [B * NH * S] rowsum(dO * O)
  float* drel_part;         // bwd workspace (REL): [B * NH][nkb][1024] bias-gradient partials per key block
  float* drel;              // bwd: [B * NH][1024], added to
  int nqb, nkb;             // query / key blocks of 128 per (sample, head) in the grid
};
}  // namespace attn_long

// packed: sample b's `len` tokens start at row cu[b]; tiles may run past them into rows of the next sample (finite data, masked as
// keys, never stored as queries)
__device__ __forceinline__ void sample_rows(const AttnCommon& p, int b, long& row0, int& len) {
  row0 = p.cu ? (long)p.cu[b] : (long)b * p.S;
  len = p.cu ? (p.cu[b + 1] - p.cu[b]) : p.S;
}

// ------------------------------------------------------------------------------------------------ blocks of the forward kernels
// One 32-key tile of the softmax.  x: the tile's log2-domain scores of this lane's query; they become exp2(x - m) times the dropout
// multiplier, and the undropped values are added to lsum.  Keys acc32_row(r), acc32_row(r + 1) are an aligned pair: one hash for both.
// e0: dropout_hash2's argument for the tile's first key on this lane (32-bit wrap-around arithmetic, as the element index is defined;
// even, because S and the offset are: attn_prepare).
template <bool DROP>
__device__ __forceinline__ void exp2_dropout_tile(f32x16& x, float m, float& lsum, uint32_t e0, const Dropout& drop) {
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const float p0 = __builtin_amdgcn_exp2f(x[r] - m), p1 = __builtin_amdgcn_exp2f(x[r + 1] - m);
    lsum += p0; lsum += p1;
    float d0 = 1.0f, d1 = 1.0f;
    if constexpr (DROP) {       // (a template parameter: tested at run time, every pair sat in its own basic block)
      const uint32_t hsh = mix32(((e0 + (uint32_t)((r & 3) + 8 * (r >> 2))) >> 1) ^ drop.key);
      d0 = dropout_pick(drop, hsh, 0u); d1 = dropout_pick(drop, hsh, 1u);
    }
    x[r] = p0 * d0; x[r + 1] = p1 * d1;
  }
}
// a wave's [32 rows][64 d] result (two 32x32 accumulators, row on the lane) times `scale` -> this lane's row, 8 bytes per store; hh: the lane's half-wave
__device__ __forceinline__ void store_row_frags(const f32x16 (&acc)[2], float scale, bf16_t* row, int hh) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = dt * 32 + 8 * i + 4 * hh;
      uint2 v = {pack2bf(acc[dt][4 * i] * scale, acc[dt][4 * i + 1] * scale), pack2bf(acc[dt][4 * i + 2] * scale, acc[dt][4 * i + 3] * scale)};
      *(uint2*)(row + d) = v;
    }
}

// ------------------------------------------------------------------------------------------------ host: the REL x DROP instances
// Both are for the int-returning launchers of the two .hip files.
// ATTN_LAUNCH: K<REL, DROP>(p) on 256 threads -- REL when p has a bias, DROP when its dropout is on; LDS / LDS_REL: dynamic LDS bytes
// without / with the bias.
#define ATTN_LAUNCH(K, grid, LDS, LDS_REL, stream, p)                                             \
  do {                                                                                            \
    const bool drop_ = (p).drop.thresh != 0;                                                      \
    if ((p).rel) {                                                                                \
      if (drop_) hipLaunchKernelGGL((K<true, true>), grid, dim3(256), LDS_REL, stream, p);        \
      else hipLaunchKernelGGL((K<true, false>), grid, dim3(256), LDS_REL, stream, p);             \
    } else {                                                                                      \
      if (drop_) hipLaunchKernelGGL((K<false, true>), grid, dim3(256), LDS, stream, p);           \
      else hipLaunchKernelGGL((K<false, false>), grid, dim3(256), LDS, stream, p);                \
    }                                                                                             \
  } while (0)
// ATTN_DYNAMIC_LDS: registers those sizes for the four instances of a backward kernel on the first call (idempotent; a benign race
// does it twice); a failure returns from the caller, so it goes before anything is launched.
#define ATTN_DYNAMIC_LDS(K, LDS, LDS_REL)                                                                                         \
  do {                                                                                                                            \
    static bool attr_set = false;                                                                                                 \
    if (!attr_set) {                                                                                                              \
      hipError_t e = hipFuncSetAttribute((const void*)K<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);          \
      if (e == hipSuccess) e = hipFuncSetAttribute((const void*)K<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS); \
      if (e == hipSuccess) e = hipFuncSetAttribute((const void*)K<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_REL);\
      if (e == hipSuccess) e = hipFuncSetAttribute((const void*)K<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_REL);\
      if (e != hipSuccess) return set_error(CAREL_ERR_HIP, "carel_attention_bwd: hipFuncSetAttribute: %s", hipGetErrorString(e)); \
      attr_set = true;                                                                                                            \
    }                                                                                                                             \
  } while (0)

}  // namespace carel
