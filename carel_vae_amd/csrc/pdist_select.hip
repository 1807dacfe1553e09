// Exact order statistics of the squared pairwise distances of one sample, without the distance matrix: carel_pdist_select (the
// median-heuristic kernel width of the two permutation tests).  The population is { D_ij : i < j }, D_ij = hsic_sqdist of
// hsic_device.h -- the value carel_hsic_gram multiplies by -1/s, bit for bit -- and the r-th smallest of its N = m (m-1) / 2 elements is
// found by a three-pass radix select on an order-preserving 32-bit key of the float, 11 / 11 / 10 bits, most significant first.
//   ps_zero_kernel       the whole workspace (state and histograms) to 0: every call rewrites all of it.
//   ps_sweep_kernel<P>   a workgroup owns one 64 x 64 tile of the upper triangle (tile row <= tile column) and, in passes 1 and 2, one
//                        SLOT (blockIdx.y): a key prefix that at least one rank is still following.  It stages the tile's 64 + 64 rows
//                        and their norms in LDS as hsic_gram_kernel does -- by construction: both call st_stage_pair of
//                        stat_tile_device.h -- recomputes the 4096 distances (in the diagonal tile only
//                        i < j counts), and adds 1 to an LDS histogram of the next 11 / 11 / 10 key bits for every element whose
//                        higher bits equal the slot's prefix; the non-empty bins then go to the slot's global histogram.  Integer
//                        atomicAdd only: the sums do not depend on the order, two runs give the same bits.
//   ps_scan_kernel<P>    one workgroup.  Per slot: an exclusive prefix sum over the bins; per rank of that slot: the bin that holds its
//                        residual rank, the residual inside the bin, `below` += the count under the bin.  Thread 0 then extends each
//                        rank's prefix and re-assigns slots -- ranks with equal prefixes share one (the two median ranks nearly always
//                        do: a sweep per DISTINCT prefix, not per rank); the workgroups of unused slots leave at once.  After pass 2
//                        the prefix is the whole key: values[q] = its float, counts[q] = (below, the bin's count = #{D == v}).
// Everything stays on the device between the passes (no read-back); seven launches.
// The key: u = bits(v); negative -> ~u, else u | 0x80000000; -0 counts as +0, and any NaN (the precondition is finite inputs) becomes
// 0xffffffff, above +inf: whatever the bits, the bin index stays inside its histogram.
// LDS per workgroup: 33 280 B rows + 512 B norms + 8 192 B histogram = 41 984 B (three workgroups per CU).
// PS_WAVE_AGGREGATE (a one-off build's flag): lanes of a wave with equal bins add once.  Off: it measured slower.
#include "carel_hip_internal.h"
#include "hsic_device.h"
#include "stat_tile_device.h"

#ifndef PS_WAVE_AGGREGATE
#define PS_WAVE_AGGREGATE 0
#endif

namespace carel {

constexpr int PS_MAX_RANKS = 8;
constexpr int PS_BINS = 2048;                // bins of passes 0 and 1 (11 bits); pass 2 uses 1024 (10 bits)
constexpr int PS_STATE_BYTES = 256;

struct PsState {                             // the head of the workspace
  unsigned n_slots, pad;
  unsigned slot_prefix[PS_MAX_RANKS];        // the key bits fixed so far, per slot
  unsigned slot_of[PS_MAX_RANKS];            // per rank
  unsigned prefix[PS_MAX_RANKS];             // per rank
  unsigned resid[PS_MAX_RANKS];              // the rank inside the elements that share the prefix
  unsigned long long below[PS_MAX_RANKS];    // #{D < every element that shares the prefix}
};
static_assert(sizeof(PsState) <= PS_STATE_BYTES, "state");

struct PsArgs {
  const float* x; long ldx; int m, d, xs, tiles, n_ranks;
  unsigned ranks[PS_MAX_RANKS];
  PsState* state;
  unsigned* hist[3];                         // [2048], [n_ranks][2048], [n_ranks][1024]
  float* values; long long* counts;
};

__device__ __forceinline__ unsigned ps_key(float v) {
  if (v != v) return 0xffffffffu;
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float ps_unkey(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }

// every lane of the wave calls (the aggregating form votes)
__device__ __forceinline__ void ps_hist_add(unsigned* hist, bool on, unsigned bin) {
#if PS_WAVE_AGGREGATE
  unsigned long long todo = __ballot(on);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned b0 = (unsigned)__shfl((int)bin, leader, 64);
    const unsigned long long same = __ballot(on && bin == b0);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[b0], (unsigned)__popcll(same));
    todo &= ~same;
  }
#else
  if (on) atomicAdd(&hist[bin], 1u);
#endif
}

__global__ __launch_bounds__(256) void ps_zero_kernel(unsigned* w, long words) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < words) w[e] = 0u;
}

template <int PASS>
__global__ __launch_bounds__(ST_THREADS) void ps_sweep_kernel(PsArgs a) {
  constexpr int BINS = PASS == 2 ? 1024 : PS_BINS;
  __shared__ float X[2 * ST_TILE * ST_XS];   // rows 0..63: the tile's rows i, 64..127: its columns j; row stride xs = d | 1
  __shared__ float nrm[2 * ST_TILE];
  __shared__ unsigned hist[BINS];
  const int t = threadIdx.x, m = a.m, d = a.d, xs = a.xs;
  const int slot = PASS == 0 ? 0 : (int)blockIdx.y;
  if (PASS != 0 && slot >= (int)a.state->n_slots) return;
  const unsigned want = PASS == 0 ? 0u : a.state->slot_prefix[slot];
  int ti = 0, rem = (int)blockIdx.x;         // the blockIdx.x-th tile of the upper triangle, row by row
  while (rem >= a.tiles - ti) { rem -= a.tiles - ti; ++ti; }
  const int i0 = ti * ST_TILE, j0 = (ti + rem) * ST_TILE;
  for (int b = t; b < BINS; b += ST_THREADS) hist[b] = 0u;
  const float* x = a.x; const long ldx = a.ldx;
  st_stage_pair(X, nrm, [=](int g) { return x + (long)g * ldx; }, i0, j0, m, d, xs);
  for (int e = t; e < ST_TILE * ST_TILE; e += ST_THREADS) {       // a wave: one row ii, 64 columns jj
    const int ii = e / ST_TILE, jj = e - ii * ST_TILE;
    const unsigned key = ps_key(hsic_sqdist(X, nrm, ii, ST_TILE + jj, d, xs));
    bool on = i0 + ii < j0 + jj && j0 + jj < m;
    unsigned bin;
    if (PASS == 0) bin = key >> 21;
    else if (PASS == 1) { on = on && (key >> 21) == want; bin = (key >> 10) & 2047u; }
    else { on = on && (key >> 10) == want; bin = key & 1023u; }
    ps_hist_add(hist, on, bin);
  }
  __syncthreads();
  unsigned* out = a.hist[PASS] + (size_t)slot * BINS;
  for (int b = t; b < BINS; b += ST_THREADS) {
    const unsigned h = hist[b];
    if (h) atomicAdd(&out[b], h);
  }
}

template <int PASS>
__global__ __launch_bounds__(256) void ps_scan_kernel(PsArgs a) {
  constexpr int BINS = PASS == 2 ? 1024 : PS_BINS, BITS = PASS == 2 ? 10 : 11, PER = BINS / 256;
  __shared__ unsigned part[256];
  __shared__ unsigned fbin[PS_MAX_RANKS], fcum[PS_MAX_RANKS], fcnt[PS_MAX_RANKS];
  PsState* st = a.state;
  const int t = threadIdx.x;
  const int n_slots = PASS == 0 ? 1 : (int)st->n_slots;
  if (t < PS_MAX_RANKS) { fbin[t] = 0u; fcum[t] = 0u; fcnt[t] = 0u; }
  for (int s = 0; s < n_slots; ++s) {
    __syncthreads();
    unsigned h[PER], sum = 0u;
#pragma unroll
    for (int p = 0; p < PER; ++p) { h[p] = a.hist[PASS][(size_t)s * BINS + t * PER + p]; sum += h[p]; }
    part[t] = sum;
    __syncthreads();
    unsigned base = 0u;
    for (int u = 0; u < t; ++u) base += part[u];
    for (int q = 0; q < a.n_ranks; ++q) {
      if ((PASS == 0 ? 0 : (int)st->slot_of[q]) != s) continue;
      const unsigned r = PASS == 0 ? a.ranks[q] : st->resid[q];
      unsigned c = base;
#pragma unroll
      for (int p = 0; p < PER; ++p) {        // exactly one bin of the slot holds r: the counts of a slot add up to more than r
        if (h[p] && r >= c && r - c < h[p]) { fbin[q] = (unsigned)(t * PER + p); fcum[q] = c; fcnt[q] = h[p]; }
        c += h[p];
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    unsigned n = 0u;
    for (int q = 0; q < a.n_ranks; ++q) {
      const unsigned pre = ((PASS == 0 ? 0u : st->prefix[q]) << BITS) | fbin[q];
      const unsigned long long below = (PASS == 0 ? 0ull : st->below[q]) + fcum[q];
      st->prefix[q] = pre;
      st->resid[q] = (PASS == 0 ? a.ranks[q] : st->resid[q]) - fcum[q];
      st->below[q] = below;
      unsigned s = 0u;
      while (s < n && st->slot_prefix[s] != pre) ++s;
      if (s == n) st->slot_prefix[n++] = pre;
      st->slot_of[q] = s;
      if (PASS == 2) {
        a.values[q] = ps_unkey(pre);
        if (a.counts) { a.counts[2 * q] = (long long)below; a.counts[2 * q + 1] = (long long)fcnt[q]; }
      }
    }
    st->n_slots = n;
  }
}

}  // namespace carel

using namespace carel;

extern "C" int64_t carel_pdist_select_workspace_bytes(int32_t m, int32_t n_ranks) {
  if (m < 2 || m > STAT_MAX_ROWS || n_ranks < 1 || n_ranks > PS_MAX_RANKS) return 0;
  // the state, then u32 histograms: pass 0 [2048], pass 1 [n_ranks][2048], pass 2 [n_ranks][1024]
  return PS_STATE_BYTES + 4 * ((int64_t)PS_BINS + (int64_t)n_ranks * (PS_BINS + 1024));
}

extern "C" int carel_pdist_select(const carel_pdist_select_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "carel_pdist_select";
  if (!a || !a->x || !a->values || !a->workspace) return set_error(CAREL_ERR_ARG, "%s: null pointer", who);
  if (a->m < 2 || a->m > STAT_MAX_ROWS) return set_error(CAREL_ERR_SHAPE, "%s: m must be in 2..%d (got %d)", who, STAT_MAX_ROWS, a->m);
  if (a->d < 1 || a->d > STAT_MAX_D) return set_error(CAREL_ERR_SHAPE, "%s: d must be in 1..%d (got %d)", who, STAT_MAX_D, a->d);
  if (a->ldx < a->d) return set_error(CAREL_ERR_ARG, "%s: row stride of x below d", who);
  if (a->n_ranks < 1 || a->n_ranks > PS_MAX_RANKS)
    return set_error(CAREL_ERR_SHAPE, "%s: n_ranks must be in 1..%d (got %d)", who, PS_MAX_RANKS, a->n_ranks);
  const int64_t N = (int64_t)a->m * (a->m - 1) / 2;
  for (int q = 0; q < a->n_ranks; ++q)
    if (a->ranks[q] < 0 || a->ranks[q] >= N)
      return set_error(CAREL_ERR_ARG, "%s: rank %lld outside [0, %lld) (m = %d)", who, (long long)a->ranks[q], (long long)N, a->m);
  const int64_t need = carel_pdist_select_workspace_bytes(a->m, a->n_ranks);
  if (int rc = check_workspace(who, a->workspace, 16, a->workspace_bytes, need)) return rc;
  PsArgs k;
  k.x = (const float*)a->x; k.ldx = a->ldx; k.m = a->m; k.d = a->d; k.xs = a->d | 1; k.n_ranks = a->n_ranks;
  k.tiles = (k.m + ST_TILE - 1) / ST_TILE;
  for (int q = 0; q < PS_MAX_RANKS; ++q) k.ranks[q] = q < k.n_ranks ? (unsigned)a->ranks[q] : 0u;      // N < 2^25
  k.state = (PsState*)a->workspace;
  k.hist[0] = (unsigned*)((char*)a->workspace + PS_STATE_BYTES);
  k.hist[1] = k.hist[0] + PS_BINS;
  k.hist[2] = k.hist[1] + (size_t)k.n_ranks * PS_BINS;
  k.values = (float*)a->values; k.counts = (long long*)a->counts;
  const long words = (long)(need / 4);
  const unsigned tri = (unsigned)(k.tiles * (k.tiles + 1) / 2);
  hipLaunchKernelGGL(ps_zero_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, (unsigned*)a->workspace, words);
  hipLaunchKernelGGL(ps_sweep_kernel<0>, dim3(tri), dim3(ST_THREADS), 0, stream, k);
  hipLaunchKernelGGL(ps_scan_kernel<0>, dim3(1), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(ps_sweep_kernel<1>, dim3(tri, (unsigned)k.n_ranks), dim3(ST_THREADS), 0, stream, k);
  hipLaunchKernelGGL(ps_scan_kernel<1>, dim3(1), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(ps_sweep_kernel<2>, dim3(tri, (unsigned)k.n_ranks), dim3(ST_THREADS), 0, stream, k);
  hipLaunchKernelGGL(ps_scan_kernel<2>, dim3(1), dim3(256), 0, stream, k);
  return check_launch("carel_pdist_select");
}
