// kernels_weighted_sweep.hip — the sweep cut by relationship weight (include/pprhip.h "weighted local clustering";
// DESIGN.md §2 "Weighted sweep cut").  The weights enter as integers in fixed point: q(e) = max(1, rint(w(e) * 2^s)) with
// the shift s of pprhip_weight_quantum, so that every sum of the sweep is a 64-bit integer and the result the same
// words every run, as the unweighted sweep's is.  The slot space, the tiles and the order of the steps are those of
// kernels_sweep.hip, whose kernels stay as they are; its sorts, scans, k_sweep_tile_starts and k_sweep_best(_final) are
// called unchanged (they do not care what their u64 arrays count).  This file's own kernels:
//   k_wsweep_wmax     once per weight set: the largest of the m weights (it fixes s)
//   k_wsweep_qdeg     once per weight set: qdeg[v] = the quanta of v's out-row plus in-row, and their total
//   k_wsweep_qdeg_hubs  ... the rows of kQdegHubRow entries or more, each summed by the whole grid
//   k_wsweep_support  k_sweep_support with the score x(v) / (double)qdeg[v]
//   k_wsweep_rank     k_sweep_rank, plus qdeg per position (its scan is the volume in quanta)
//   k_wsweep_edges    THE HOT KERNEL: k_sweep_edges adding +q / -q per slot, every sum in 64 bits
#include <algorithm>

#include "device_utils.hpp"
#include "engine.hpp"

namespace pprhip {

typedef unsigned long long u64;

constexpr int kSweepPerThread = (int)(kSweepTile / 256u);  // slots a thread takes per tile, 256 apart (lane-contiguous)
constexpr uint32_t kQdegWaveRow = 32;  // rows of so many entries or more are summed by the whole wave
static_assert(kQdegHubRow >= 2 * kSweepTile, "the hub list lives in SweepWs::tile_node: two words per row of kQdegHubRow entries");

// the quantum of a weight: ldexp by an integer is exact, the rounding is to nearest, ties to even; a weight below half a
// quantum counts as one (w * 2^s < 2^61: the conversion cannot overflow)
__device__ __forceinline__ u64 wsweep_quantum(double w, int shift) {
  const long long q = __double2ll_rn(ldexp(w, shift));
  return q < 1 ? 1ull : (u64)q;
}

// ------------------------------------------------------------------ once per weight set
__global__ __launch_bounds__(256) void k_wsweep_wmax(const double* __restrict__ out_w, u64 m, u64* __restrict__ cell) {
  __shared__ u64 s_max[4];
  u64 best = 0;
  for (u64 e = blockIdx.x * 256ull + threadIdx.x; e < m; e += (u64)gridDim.x * 256ull) {
    const u64 b = (u64)__double_as_longlong(out_w[e]);
    best = b > best ? b : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = __shfl_down(best, o);
    best = t > best ? t : best;
  }
  if (lane_id() == 0) s_max[wave_id()] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) best = s_max[w] > best ? s_max[w] : best;
    if (best) (void)__hip_atomic_fetch_max(cell, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the quanta of one row, summed by the whole wave (coalesced, 64 entries per step); valid in every lane
__device__ __forceinline__ u64 wsweep_row_by_wave(const double* __restrict__ w, uint32_t begin, uint32_t len, int shift) {
  u64 s = 0;
  for (uint32_t k = (uint32_t)lane_id(); k < len; k += 64u) s += wsweep_quantum(w[(u64)begin + k], shift);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

// One lane per node and a wave per 64 consecutive nodes.  A lane sums its node's short rows itself; the rows of
// kQdegWaveRow entries or more are taken one after another by the whole wave, so that no lane walks a long row alone;
// the rows of kQdegHubRow entries or more (the internal order puts the largest out-degrees side by side: one wave would
// get them all) are listed as (node, 0: out-row / 1: in-row) for k_wsweep_qdeg_hubs.  Integer sums: any order gives the
// same words.
__global__ __launch_bounds__(256) void k_wsweep_qdeg(uint32_t n, const uint32_t* __restrict__ out_rp,
                                                      const uint32_t* __restrict__ in_rp,
                                                      const double* __restrict__ out_w, const double* __restrict__ in_w,
                                                      int shift, u64* __restrict__ qdeg, u64* __restrict__ total,
                                                      uint32_t* __restrict__ hub_list, u64* __restrict__ hub_count) {
  const uint32_t stride = gridDim.x * 256u;
  const uint32_t nround = (n + stride - 1u) / stride * stride;
  const int lane = lane_id();
  u64 mine = 0;
  for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < nround; v += stride) {
    uint32_t ob = 0, ol = 0, ib = 0, il = 0;
    if (v < n) {
      ob = out_rp[v];
      ol = out_rp[v + 1] - ob;
      ib = in_rp[v];
      il = in_rp[v + 1] - ib;
    }
    u64 s = 0;
    if (ol < kQdegWaveRow)
      for (uint32_t k = 0; k < ol; ++k) s += wsweep_quantum(out_w[(u64)ob + k], shift);
    if (il < kQdegWaveRow)
      for (uint32_t k = 0; k < il; ++k) s += wsweep_quantum(in_w[(u64)ib + k], shift);
    if (ol >= kQdegHubRow) {  // (at most 2m / kQdegHubRow rows are that long: the list has room for them)
      const u64 at = atomic_add_u64(hub_count, 1ull);
      hub_list[2 * at] = v;
      hub_list[2 * at + 1] = 0u;
    }
    if (il >= kQdegHubRow) {
      const u64 at = atomic_add_u64(hub_count, 1ull);
      hub_list[2 * at] = v;
      hub_list[2 * at + 1] = 1u;
    }
    for (u64 mask = __ballot(ol >= kQdegWaveRow && ol < kQdegHubRow); mask; mask &= mask - 1ull) {
      const int l = __ffsll((long long)mask) - 1;
      const u64 r = wsweep_row_by_wave(out_w, __shfl(ob, l), __shfl(ol, l), shift);
      if (lane == l) s += r;
    }
    for (u64 mask = __ballot(il >= kQdegWaveRow && il < kQdegHubRow); mask; mask &= mask - 1ull) {
      const int l = __ffsll((long long)mask) - 1;
      const u64 r = wsweep_row_by_wave(in_w, __shfl(ib, l), __shfl(il, l), shift);
      if (lane == l) s += r;
    }
    if (v < n) {
      qdeg[v] = s;
      mine += s;
    }
  }
  mine = wave_sum_u64(mine);
  if (lane == 0 && mine) (void)atomic_add_u64(total, mine);
}

// the listed hub rows, one after another, each by the whole grid: a workgroup adds its share of the row to the node's
// qdeg (written by k_wsweep_qdeg without that row) and to the total with one atomic each
__global__ __launch_bounds__(256) void k_wsweep_qdeg_hubs(const uint32_t* __restrict__ hub_list,
                                                           const u64* __restrict__ hub_count,
                                                           const uint32_t* __restrict__ out_rp,
                                                           const uint32_t* __restrict__ in_rp,
                                                           const double* __restrict__ out_w,
                                                           const double* __restrict__ in_w, int shift,
                                                           u64* __restrict__ qdeg, u64* __restrict__ total) {
  __shared__ u64 s_part[4];
  const u64 nh = *hub_count;
  for (u64 h = 0; h < nh; ++h) {
    const uint32_t v = hub_list[2 * h];
    const bool in_row = hub_list[2 * h + 1] != 0u;
    const uint32_t* rp = in_row ? in_rp : out_rp;
    const double* w = in_row ? in_w : out_w;
    const uint32_t begin = rp[v], len = rp[v + 1] - begin;
    u64 s = 0;
    for (u64 k = blockIdx.x * 256ull + threadIdx.x; k < len; k += (u64)gridDim.x * 256ull)
      s += wsweep_quantum(w[(u64)begin + k], shift);
    s = block_sum_u64(s, s_part);  // (valid in thread 0)
    if (threadIdx.x == 0 && s) {
      (void)atomic_add_u64(&qdeg[v], s);
      (void)atomic_add_u64(total, s);
    }
  }
}

// ------------------------------------------------------------------ 1. support
// a node with an adjacency slot has qdeg >= 1 (no quantum is 0), a node without one has qdeg = 0
__global__ __launch_bounds__(256) void k_wsweep_support(const double* __restrict__ x, uint32_t n,
                                                         const u64* __restrict__ qdeg,
                                                         const int32_t* __restrict__ new2old, int normalize,
                                                         u64* __restrict__ keys, uint32_t* __restrict__ ids,
                                                         u64* __restrict__ count) {
  const uint32_t stride = gridDim.x * 256u;
  const uint32_t nround = (n + stride - 1u) / stride * stride;
  const int lane = lane_id();
  for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < nround; v += stride) {
    bool take = false;
    u64 key = 0;
    if (v < n) {
      const double xv = x[v];
      if (xv > 0.0) {
        const u64 d = qdeg[v];
        if (d) {
          const double s = normalize ? xv / (double)d : xv;
          key = ~(u64)__double_as_longlong(s);
          take = true;
        }
      }
    }
    const u64 mask = __ballot(take);
    if (mask == 0) continue;
    const int leader = __ffsll((long long)mask) - 1;
    u64 base = 0;
    if (lane == leader) base = atomic_add_u64(count, (u64)__popcll(mask));
    base = __shfl(base, leader);
    if (take) {
      const u64 pos = base + (u64)__popcll(mask & ((1ull << lane) - 1ull));  // (< n: every node is taken at most once)
      keys[pos] = key;
      ids[pos] = (uint32_t)new2old[v];
    }
  }
}

// ------------------------------------------------------------------ 3. rank table, row extents, both degrees
__global__ __launch_bounds__(256) void k_wsweep_rank(const uint32_t* __restrict__ order, uint32_t profiled,
                                                      const int32_t* __restrict__ old2new,
                                                      const uint32_t* __restrict__ out_rp,
                                                      const uint32_t* __restrict__ in_rp, const u64* __restrict__ qdeg,
                                                      uint32_t* __restrict__ rank, uint4* __restrict__ rec,
                                                      u64* __restrict__ deg, u64* __restrict__ volx,
                                                      u64* __restrict__ qd, u64* __restrict__ qvolx) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    volx[0] = 0ull;
    qvolx[0] = 0ull;
  }
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < profiled; i += gridDim.x * 256u) {
    const uint32_t v = (uint32_t)old2new[order[i]];
    const uint32_t ob = out_rp[v], d_out = out_rp[v + 1] - ob;
    const uint32_t ib = in_rp[v], d_in = in_rp[v + 1] - ib;
    rank[v] = i;
    rec[i] = make_uint4(v, ob, d_out, ib);
    deg[i] = (u64)d_out + (u64)d_in;
    qd[i] = qdeg[v];
  }
}

// ------------------------------------------------------------------ 4. the edge scan
// k_sweep_edges' turn over a tile of kSweepTile slots (the tiles are those of the count degree: volx, tile_node and
// the search in LDS are the same), with the slot's weight streamed beside its column index - out_w at the out-row
// offset, in_w at the in-row offset, both coalesced like the indices - and +q / -q added where that kernel adds +1 / -1.
// A partial sum is near 2^(61 - L) from the first slot on, so everything that carries one is 64 bits wide: the
// register run, the node's LDS cell (32 KB of cells beside the 16 KB of starts: three workgroups share a CU), the wave
// reduction, the store and the atomic of the nodes that cross a tile boundary.
__global__ __launch_bounds__(256) void k_wsweep_edges(const u64* __restrict__ volx, uint32_t profiled,
                                                       const uint32_t* __restrict__ tile_node,
                                                       const uint4* __restrict__ rec, const uint32_t* __restrict__ rank,
                                                       const int32_t* __restrict__ out_ci,
                                                       const int32_t* __restrict__ in_ci,
                                                       const double* __restrict__ out_w, const double* __restrict__ in_w,
                                                       int shift, long long* __restrict__ delta, u64* __restrict__ hdr) {
  __shared__ uint32_t s_start[kSweepTile];
  __shared__ u64 s_delta[kSweepTile];
  const u64 total = volx[profiled];
  const u64 n_tiles = (total + kSweepTile - 1) / kSweepTile;
  const int lane = lane_id();
  if (blockIdx.x == 0 && threadIdx.x == 0) hdr[6] = total;  // the edge slots scanned
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 t0 = t * kSweepTile;
    const u64 t1 = t0 + kSweepTile < total ? t0 + kSweepTile : total;
    const uint32_t i0 = tile_node[t];
    uint32_t i_last = profiled - 1u;
    if (t + 1 < n_tiles) {  // the node that holds slot t1 - 1
      const uint32_t nx = tile_node[t + 1];
      i_last = volx[nx] < t1 ? nx : nx - 1u;
    }
    const uint32_t cnt = i_last - i0 + 1u;  // (<= kSweepTile: every node of the tile holds a slot of it)
    const u64 first_start = volx[i0];       // (<= t0)
    for (uint32_t j = threadIdx.x; j < cnt; j += 256u) {
      const u64 st = volx[i0 + j];
      s_start[j] = st > t0 ? (uint32_t)(st - t0) : 0u;
      s_delta[j] = 0ull;
    }
    __syncthreads();
    int cur_j = -1;
    u64 acc = 0;  // two's complement: -q is added as its u64 image
#pragma unroll 4
    for (int k = 0; k < kSweepPerThread; ++k) {
      const uint32_t ls = (uint32_t)k * 256u + threadIdx.x;
      const u64 s = t0 + ls;
      if (s < t1) {
        uint32_t lo = 0, hi = cnt;  // s_start[lo] <= ls < s_start[hi]
        while (hi - lo > 1) {       // (the same trip count in every lane)
          const uint32_t mid = (lo + hi) >> 1;
          if (s_start[mid] <= ls) lo = mid;
          else hi = mid;
        }
        const uint32_t i = i0 + lo;
        const uint4 rc = rec[i];  // node, out-row begin, out-degree, in-row begin
        const u64 o = lo == 0 ? s - first_start : (u64)(ls - s_start[lo]);
        const bool in_row = o >= (u64)rc.z;
        const u64 at = in_row ? (u64)rc.w + (o - (u64)rc.z) : (u64)rc.y + o;
        const int32_t u = in_row ? in_ci[at] : out_ci[at];
        const double wt = in_row ? in_w[at] : out_w[at];
        const uint32_t r = rank[u];
        const u64 q = wsweep_quantum(wt, shift);
        const u64 c = (uint32_t)u == rc.x ? 0ull : (r > i ? q : 0ull - q);
        if ((int)lo != cur_j) {
          if (cur_j >= 0 && acc) atomicAdd(&s_delta[cur_j], acc);
          cur_j = (int)lo;
          acc = 0;
        }
        acc += c;
      }
    }
    {
      const int j0 = __shfl(cur_j, 0);
      if (__all(cur_j == j0)) {  // the whole wave ended on one node (a hub's tile): one LDS add per wave
        const u64 sum = wave_sum_u64(acc);
        if (lane == 0 && j0 >= 0 && sum) atomicAdd(&s_delta[j0], sum);
      } else if (cur_j >= 0 && acc) {
        atomicAdd(&s_delta[cur_j], acc);
      }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < cnt; j += 256u) {
      const uint32_t i = i0 + j;
      const u64 d = s_delta[j];
      const bool inside = (j > 0 || first_start >= t0) && (j + 1u < cnt || volx[i + 1] <= t1);
      if (inside) delta[i] = (long long)d;
      else if (d) (void)atomic_add_u64(reinterpret_cast<u64*>(&delta[i]), d);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ launchers
int launch_wsweep_wmax(pprhip_graph* g, u64* cell) {
  const GraphData* D = g->gr;
  if (D->m == 0) return PPRHIP_OK;
  hipLaunchKernelGGL(k_wsweep_wmax, dim3(sweep_item_grid(D->m, (uint32_t)D->n_cus * 8u)), dim3(256), 0, g->stream, D->out_w,
                     (u64)D->m, cell);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_wsweep_qdeg(pprhip_graph* g, SweepWs* w, int shift, u64* qdeg, u64* total, u64* hub_count) {
  const GraphData* D = g->gr;
  hipLaunchKernelGGL(k_wsweep_qdeg, dim3(sweep_item_grid(D->n, (uint32_t)D->n_cus * 8u)), dim3(256), 0, g->stream, D->n,
                     D->out_rp, D->in_rp, D->out_w, D->in_w, shift, qdeg, total, w->tile_node, hub_count);
  const uint32_t hub_grid = (uint32_t)D->n_cus * 4u;
  hipLaunchKernelGGL(k_wsweep_qdeg_hubs, dim3(sweep_item_grid(256ull * hub_grid, hub_grid)), dim3(256), 0, g->stream,
                     w->tile_node, hub_count, D->out_rp, D->in_rp, D->out_w, D->in_w, shift, qdeg, total);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_wsweep_support(pprhip_graph* g, SweepWs* w, const double* x, int normalize) {
  const GraphData* D = g->gr;
  PPRHIP_CHECK_HIP(hipMemsetAsync(w->hdr, 0, sizeof(u64) * kSweepHdrWords, g->stream));
  hipLaunchKernelGGL(k_wsweep_support, dim3(sweep_item_grid(D->n, 2048)), dim3(256), 0, g->stream, x, D->n, D->qdeg, D->new2old,
                     normalize, w->key[0], w->id[0], w->hdr);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// rank[v] = position for the first `profiled` positions ("none" elsewhere), the positions' row extents, vol in slots
// (w->volx) and in quanta (w->qvolx; the positions' qdeg are staged in w->cut, which the edge scan's result replaces)
int launch_wsweep_rank(pprhip_graph* g, SweepWs* w, uint32_t profiled) {
  const GraphData* D = g->gr;
  PPRHIP_CHECK_HIP(hipMemsetAsync(w->rank, 0xFF, sizeof(uint32_t) * (size_t)D->n, g->stream));  // kSweepNone
  hipLaunchKernelGGL(k_wsweep_rank, dim3(sweep_item_grid(profiled, 2048)), dim3(256), 0, g->stream, w->order, profiled,
                     D->old2new, D->out_rp, D->in_rp, D->qdeg, w->rank, w->rec, w->deg, w->volx, w->cut, w->qvolx);
  PPRHIP_CHECK_HIP(hipGetLastError());
  PPRHIP_TRY(sweep_scan(g, w, w->deg, w->volx + 1, profiled));
  return sweep_scan(g, w, w->cut, w->qvolx + 1, profiled);
}

// delta over the slot space, then cut = its scan
int launch_wsweep_edges(pprhip_graph* g, SweepWs* w, uint32_t profiled, hipEvent_t before, hipEvent_t after) {
  const GraphData* D = g->gr;
  const uint64_t max_tiles = std::max<uint64_t>(1, (2 * D->m + kSweepTile - 1) / kSweepTile);  // (<= w->tile_cap)
  PPRHIP_TRY(launch_sweep_tile_starts(g, w, profiled));
  PPRHIP_CHECK_HIP(hipEventRecord(before, g->stream));
  PPRHIP_CHECK_HIP(hipMemsetAsync(w->delta, 0, sizeof(long long) * (size_t)profiled, g->stream));
  // 48 KB of LDS per workgroup: three of them share a CU
  const uint32_t grid =
      sweep_edge_grid((uint32_t)std::min<uint64_t>(max_tiles, (uint64_t)D->n_cus * 3u));
  hipLaunchKernelGGL(k_wsweep_edges, dim3(grid), dim3(256), 0, g->stream, w->volx, profiled, w->tile_node, w->rec, w->rank,
                     D->out_ci, D->in_ci, D->out_w, D->in_w, D->q_shift, w->delta, w->hdr);
  PPRHIP_CHECK_HIP(hipGetLastError());
  PPRHIP_CHECK_HIP(hipEventRecord(after, g->stream));
  return sweep_scan(g, w, reinterpret_cast<const u64*>(w->delta), w->cut, profiled);
}

int init_kernels_weighted_sweep() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_wsweep_edges)));
  return PPRHIP_OK;
}

}  // namespace pprhip
