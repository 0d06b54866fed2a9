// weighted_device.hpp — device helpers the two weighted kernel files share (kernels_weighted.hip: forward levels and
// walks; kernels_weighted_bwd.hip: backward levels, survival, pair walks): the crossing list of a sparse tile and its
// append, a lane's share of a dense chunk with the weight stream, and the weighted walker.  For .hip files only.
#pragma once
#include "push_device.hpp"

namespace pprhip {

constexpr int kWTile = 2048;   // edges per workgroup iteration of k_w_push
constexpr int kWStage = 512;   // frontier entries staged in LDS at a time

struct WNewList {  // crossings of the current tile, collected in LDS
  int32_t node[kWTile + 1];
  uint32_t deg[kWTile + 1];
  uint32_t count;
};

// the unweighted push test on (old, old + add): the relationship count, whatever the weights are; a crossing joins the
// tile's list
__device__ __forceinline__ void w_push_finish(int32_t u, double add, double old, uint32_t du, WNewList* nl, double rmax) {
  const double nw = old + add;
  if (!active_fwd(old, du, rmax) && active_fwd(nw, du, rmax)) {
    const uint32_t slot = atomicAdd(&nl->count, 1u);
    nl->node[slot] = u;
    nl->deg[slot] = du;
  }
}

// Appends the tile's crossings to the next frontier: one packed atomic reserves list slots and the edge range, a
// workgroup scan turns the degrees into edge offsets (kernels_push.hip: flush_new).
__device__ __forceinline__ void w_flush_new(WNewList* nl, int32_t* __restrict__ Fn, uint32_t* __restrict__ eoffn,
                                            unsigned long long* out_counter) {
  __shared__ unsigned long long s_scan[4];
  __shared__ unsigned long long s_base;
  __syncthreads();
  const uint32_t cnt = nl->count;
  if (cnt == 0) return;  // uniform
  const int tid = threadIdx.x;
  constexpr int kPer = (kWTile + 1 + 255) / 256;
  const uint32_t b = tid * kPer;
  unsigned long long mine = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (b + j < cnt) mine += nl->deg[b + j];
  unsigned long long total = 0;
  const unsigned long long excl = block_excl_scan_256<unsigned long long>(mine, s_scan, &total);
  if (tid == 0) s_base = atomic_add_u64(out_counter, ((unsigned long long)cnt << kPackShift) | total);
  __syncthreads();
  const uint32_t pos0 = (uint32_t)(s_base >> kPackShift);
  unsigned long long e = (s_base & kPackMask) + excl;
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (b + j < cnt) {
      Fn[pos0 + b + j] = nl->node[b + j];
      eoffn[pos0 + b + j] = (uint32_t)e;
      e += nl->deg[b + j];
    }
  __syncthreads();
  if (tid == 0) nl->count = 0;
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// dense level: a lane's registers of one chunk
// ------------------------------------------------------------------------------------------------
struct WChunkRegs {  // one lane's share of a chunk: 8 column indices, their weights and their row-start flags
  int4 ia, ib;
  double w[8];
  uint32_t fb;
};

__device__ __forceinline__ WChunkRegs w_load_chunk(const int32_t* __restrict__ in_ci, const double* __restrict__ in_w,
                                                   const uint8_t* __restrict__ start_flags, uint32_t c, int lane) {
  const unsigned long long e0 = (unsigned long long)c * kChunkEdges + 8ull * lane;
  // both streams are read once per sweep: non-temporal, so that they do not push gathered lines out of L2
  typedef int v4i __attribute__((ext_vector_type(4)));
  typedef double v2d __attribute__((ext_vector_type(2)));
  const v4i* q = reinterpret_cast<const v4i*>(in_ci + e0);
  const v2d* qw = reinterpret_cast<const v2d*>(in_w + e0);
  const v4i x = __builtin_nontemporal_load(q), y = __builtin_nontemporal_load(q + 1);
  const v2d w0 = __builtin_nontemporal_load(qw), w1 = __builtin_nontemporal_load(qw + 1),
            w2 = __builtin_nontemporal_load(qw + 2), w3 = __builtin_nontemporal_load(qw + 3);
  WChunkRegs r;
  r.ia = make_int4(x.x, x.y, x.z, x.w);
  r.ib = make_int4(y.x, y.y, y.z, y.w);
  r.w[0] = w0.x; r.w[1] = w0.y; r.w[2] = w1.x; r.w[3] = w1.y;
  r.w[4] = w2.x; r.w[5] = w2.y; r.w[6] = w3.x; r.w[7] = w3.y;
  r.fb = __builtin_nontemporal_load(&start_flags[e0 >> 3]);
  return r;
}

// ------------------------------------------------------------------------------------------------
// weighted walks
// ------------------------------------------------------------------------------------------------
struct WPhilox {
  uint32_t x[4];
};

__device__ __forceinline__ WPhilox w_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                   uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  WPhilox p;
  p.x[0] = c0; p.x[1] = c1; p.x[2] = c2; p.x[3] = c3;
  return p;
}

// the arrays a weighted walk reads
struct WWalkGraph {
  const unsigned long long* out_ext;
  const int32_t* out_ci;
  const double* out_cum;
  const double* wsum;
};

// Per-lane walk state machine (kernels_walk.hip: Walker): same counter, key and word use; one decision per step.
struct WWalker {
  int32_t start, cur;
  uint32_t c0, c1, c2;  // counter words 0-2 (original id of the start node, walk index, stream)
  uint32_t k;           // next decision number
  uint32_t w_stop2, w_pick2;  // second half of the cached Philox block
  uint32_t moves;
  bool forced;          // the next decision is the forced first hop (no_zero_hop)
  uint32_t b, d;        // out-row of the current node: first edge, degree
  uint32_t sb, sd;      // the same for the start node
};

__device__ __forceinline__ void w_walker_init(WWalker& w, int32_t start, unsigned long long start_ext, int32_t start_orig,
                                              unsigned long long idx, uint32_t stream, bool no_zero_hop) {
  w.start = start;
  w.cur = start;
  w.b = w.sb = (uint32_t)start_ext;
  w.d = w.sd = (uint32_t)(start_ext >> 32);
  w.c0 = (uint32_t)start_orig;
  w.c1 = (uint32_t)idx;
  w.c2 = (uint32_t)((idx >> 32) & 0xFFFFu) | (stream << 16);
  w.k = 0;
  w.moves = 0;
  w.forced = no_zero_hop;
}

// Returns true when the walk has stopped (w.cur is the terminal).  The pick: ceil(log2 d) dependent loads of the row's
// prefix, then the neighbour and its row extent.
__device__ __forceinline__ bool w_walker_step(WWalker& w, const WWalkGraph& G, double alpha, uint32_t k0, uint32_t k1) {
  uint32_t ws, wp;
  if ((w.k & 1u) == 0) {
    const WPhilox p = w_philox4x32_10(w.c0, w.c1, w.c2, w.k >> 1, k0, k1);
    ws = p.x[0];
    wp = p.x[1];
    w.w_stop2 = p.x[2];
    w.w_pick2 = p.x[3];
  } else {
    ws = w.w_stop2;
    wp = w.w_pick2;
  }
  w.k++;
  if (!w.forced) {
    if ((double)ws * (1.0 / 4294967296.0) < alpha) return true;
  }
  w.forced = false;
  if (w.d > 0) {
    const double x = ((double)wp * (1.0 / 4294967296.0)) * G.wsum[w.cur];
    const double* __restrict__ cum = G.out_cum + w.b;
    uint32_t lo = 0, hi = w.d;  // lo = entries of the prefix that are <= x
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (cum[mid] <= x) lo = mid + 1; else hi = mid;
    }
    const uint32_t j = lo < w.d ? lo : w.d - 1u;
    const int32_t nx = G.out_ci[w.b + j];
    const unsigned long long ext = G.out_ext[nx];
    w.cur = nx;
    w.b = (uint32_t)ext;
    w.d = (uint32_t)(ext >> 32);
  } else {  // dead end: restart at the walk's start node
    w.cur = w.start;
    w.b = w.sb;
    w.d = w.sd;
  }
  w.moves++;
  return false;
}

}  // namespace pprhip
