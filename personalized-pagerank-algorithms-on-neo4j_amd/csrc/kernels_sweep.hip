// kernels_sweep.hip — sweep cut over a PPR vector (PageRank-Nibble's second half; DESIGN.md §2 "Sweep cut").
//
// The vector's support is ordered by score (x(v) / deg(v), or x(v)), and for every prefix of that order the volume and
// the cut are computed: vol[i] = sum of deg over positions 0..i, cut[i] = relationships with exactly one endpoint among
// them.  The graph is read as undirected: deg(v) = d_out(v) + d_in(v), a node's adjacency is its out-row followed by its
// in-row, one SLOT per entry.  The cut comes from a +1 / -1 form that needs no atomic on another node's cell: the slot
// (v at position i, other endpoint u) adds +1 to delta[i] when rank[u] > i (unranked: "none" > every position), -1 when
// rank[u] < i, 0 when u == v; cut = inclusive scan of delta.  A relationship between two ranked nodes is met from both
// endpoints' rows: +1 at the lower position, -1 at the higher one - exactly the prefixes it cuts.
//   k_sweep_support      the ranked nodes' sort keys (inverted score bits) and original ids, compacted by wave ballot
//   (rocPRIM)            two stable radix sorts, by original id, then by key: score descending, ties by id ascending
//   k_sweep_rank         rank[v] = position, per position the node's row extents and deg; (rocPRIM) scan -> vol
//   k_sweep_tile_starts  first node of every tile of kSweepTile slots: binary search in the exclusive vol
//   k_sweep_edges        THE HOT KERNEL: segmented sum of the +1 / -1 over the slot space, tile by tile
//   (rocPRIM)            scan of delta -> cut
//   k_sweep_best(_final) conductance per prefix, min-reduction (ties to the shortest prefix), header for the host
// The sorts and scans are library calls (as in kernels_sort.hip); all sums are integers: the same result every run.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "device_utils.hpp"
#include "engine.hpp"

namespace pprhip {

typedef unsigned long long u64;

constexpr int kSweepPerThread = (int)(kSweepTile / 256u);  // slots a thread takes per tile, 256 apart (lane-contiguous)

// ------------------------------------------------------------------ 1. support
// key = ~bits(score): positive doubles order like their bit patterns, so ascending keys are descending scores
__global__ __launch_bounds__(256) void k_sweep_support(const double* __restrict__ x, uint32_t n,
                                                        const uint32_t* __restrict__ out_rp,
                                                        const uint32_t* __restrict__ in_rp,
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
        const u64 d = (u64)(out_rp[v + 1] - out_rp[v]) + (u64)(in_rp[v + 1] - in_rp[v]);
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

// ------------------------------------------------------------------ 3. rank table, row extents, degrees
__global__ __launch_bounds__(256) void k_sweep_rank(const uint32_t* __restrict__ order, uint32_t profiled,
                                                     const int32_t* __restrict__ old2new,
                                                     const uint32_t* __restrict__ out_rp,
                                                     const uint32_t* __restrict__ in_rp, uint32_t* __restrict__ rank,
                                                     uint4* __restrict__ rec, u64* __restrict__ deg,
                                                     u64* __restrict__ volx) {
  if (blockIdx.x == 0 && threadIdx.x == 0) volx[0] = 0ull;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < profiled; i += gridDim.x * 256u) {
    const uint32_t v = (uint32_t)old2new[order[i]];
    const uint32_t ob = out_rp[v], d_out = out_rp[v + 1] - ob;
    const uint32_t ib = in_rp[v], d_in = in_rp[v + 1] - ib;
    rank[v] = i;
    rec[i] = make_uint4(v, ob, d_out, ib);
    deg[i] = (u64)d_out + (u64)d_in;
  }
}

// tile t covers the slots [t * kSweepTile, ...): its first node is the largest i with volx[i] <= t * kSweepTile
// (volx is strictly increasing: every ranked node has deg > 0)
__global__ __launch_bounds__(256) void k_sweep_tile_starts(const u64* __restrict__ volx, uint32_t profiled,
                                                            uint32_t* __restrict__ tile_node) {
  const u64 total = volx[profiled];
  const u64 n_tiles = (total + kSweepTile - 1) / kSweepTile;
  for (u64 t = blockIdx.x * 256ull + threadIdx.x; t < n_tiles; t += (u64)gridDim.x * 256ull) {
    const u64 s = t * kSweepTile;
    uint32_t lo = 0, hi = profiled;  // volx[lo] <= s < volx[hi]
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (volx[mid] <= s) lo = mid;
      else hi = mid;
    }
    tile_node[t] = lo;
  }
}

// ------------------------------------------------------------------ 4. the edge scan
// One tile of kSweepTile consecutive slots per workgroup turn.  The nodes a tile touches are the consecutive positions
// i0 .. i0 + cnt - 1 (cnt <= kSweepTile); their first slots relative to the tile sit in LDS, a slot finds its node by
// binary search there (no search when the tile lies inside one hub).  Lane l of a turn takes slot l, l + 256, ...:
// the column indices are streamed coalesced, rank[u] is the one random gather per slot.  A thread keeps the sum of a
// run of slots of one node in a register; sums go to the node's LDS cell, a wave whose lanes all ended on the same node
// adds them up first.  Nodes inside the tile store their delta; the (at most two) nodes that cross a tile boundary add
// their partial with one 64-bit atomic.
// (k_wsweep_edges in kernels_weighted_sweep.hip is this kernel's twin with a weight stream and 64-bit sums: the tile,
// search and boundary logic is the same text there, and a fix to it here belongs there too.)
__global__ __launch_bounds__(256) void k_sweep_edges(const u64* __restrict__ volx, uint32_t profiled,
                                                      const uint32_t* __restrict__ tile_node,
                                                      const uint4* __restrict__ rec, const uint32_t* __restrict__ rank,
                                                      const int32_t* __restrict__ out_ci,
                                                      const int32_t* __restrict__ in_ci, long long* __restrict__ delta) {
  __shared__ uint32_t s_start[kSweepTile];
  __shared__ int s_delta[kSweepTile];
  const u64 total = volx[profiled];
  const u64 n_tiles = (total + kSweepTile - 1) / kSweepTile;
  const int lane = lane_id();
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 t0 = t * kSweepTile;
    const u64 t1 = t0 + kSweepTile < total ? t0 + kSweepTile : total;
    const uint32_t i0 = tile_node[t];
    uint32_t i_last = profiled - 1u;
    if (t + 1 < n_tiles) {  // the node that holds slot t1 - 1
      const uint32_t nx = tile_node[t + 1];
      i_last = volx[nx] < t1 ? nx : nx - 1u;
    }
    const uint32_t cnt = i_last - i0 + 1u;
    const u64 first_start = volx[i0];  // (<= t0)
    for (uint32_t j = threadIdx.x; j < cnt; j += 256u) {
      const u64 st = volx[i0 + j];
      s_start[j] = st > t0 ? (uint32_t)(st - t0) : 0u;
      s_delta[j] = 0;
    }
    __syncthreads();
    int cur_j = -1, acc = 0;
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
        const int32_t u = o < (u64)rc.z ? out_ci[(u64)rc.y + o] : in_ci[(u64)rc.w + (o - (u64)rc.z)];
        const uint32_t r = rank[u];
        const int c = (uint32_t)u == rc.x ? 0 : (r > i ? 1 : -1);
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
        int sum = acc;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
        if (lane == 0 && j0 >= 0 && sum) atomicAdd(&s_delta[j0], sum);
      } else if (cur_j >= 0 && acc) {
        atomicAdd(&s_delta[cur_j], acc);
      }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < cnt; j += 256u) {
      const uint32_t i = i0 + j;
      const int d = s_delta[j];
      const bool inside = (j > 0 || first_start >= t0) && (j + 1u < cnt || volx[i + 1] <= t1);
      if (inside) delta[i] = (long long)d;
      else if (d) (void)atomic_add_u64(reinterpret_cast<u64*>(&delta[i]), (u64)(long long)d);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ 5. best prefix
// candidate i: min(vol, 2m - vol) > 0 and (max_vol == 0 or vol <= max_vol); the smallest phi wins, ties go to the
// shortest prefix.  No candidate: phi = +inf, index ~0.
__device__ __forceinline__ bool sweep_better(double pa, u64 ia, double pb, u64 ib) {
  return pa < pb || (pa == pb && ia < ib);
}

__global__ __launch_bounds__(256) void k_sweep_best(const u64* __restrict__ volx, const u64* __restrict__ cut,
                                                     uint32_t profiled, u64 total_vol, u64 max_vol,
                                                     double* __restrict__ part_phi, u64* __restrict__ part_idx) {
  __shared__ double s_phi[256];
  __shared__ u64 s_idx[256];
  double best = __longlong_as_double(0x7ff0000000000000ll);
  u64 best_i = ~0ull;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < profiled; i += gridDim.x * 256u) {
    const u64 vol = volx[i + 1];
    const u64 rest = total_vol - vol;
    const u64 den = vol < rest ? vol : rest;
    if (den == 0 || (max_vol && vol > max_vol)) continue;
    const double phi = (double)cut[i] / (double)den;
    if (sweep_better(phi, i, best, best_i)) {
      best = phi;
      best_i = i;
    }
  }
  s_phi[threadIdx.x] = best;
  s_idx[threadIdx.x] = best_i;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d && sweep_better(s_phi[threadIdx.x + d], s_idx[threadIdx.x + d], s_phi[threadIdx.x], s_idx[threadIdx.x])) {
      s_phi[threadIdx.x] = s_phi[threadIdx.x + d];
      s_idx[threadIdx.x] = s_idx[threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part_phi[blockIdx.x] = s_phi[0];
    part_idx[blockIdx.x] = s_idx[0];
  }
}

// header words: [1] best_size, [2] best_cut, [3] best_vol, [4] bits of best_conductance, [5] volx[profiled] - the edge
// slots scanned when volx counts slots (the unweighted sweep); the weighted sweep passes the volume in quanta, so its
// [2], [3] and [5] are quanta and k_wsweep_edges keeps the edge slots in [6], which this kernel leaves alone
__global__ __launch_bounds__(256) void k_sweep_best_final(const double* __restrict__ part_phi,
                                                           const u64* __restrict__ part_idx, uint32_t n_part,
                                                           const u64* __restrict__ volx, const u64* __restrict__ cut,
                                                           uint32_t profiled, u64* __restrict__ hdr) {
  __shared__ double s_phi[256];
  __shared__ u64 s_idx[256];
  double best = __longlong_as_double(0x7ff0000000000000ll);
  u64 best_i = ~0ull;
  for (uint32_t p = threadIdx.x; p < n_part; p += 256u)
    if (sweep_better(part_phi[p], part_idx[p], best, best_i)) {
      best = part_phi[p];
      best_i = part_idx[p];
    }
  s_phi[threadIdx.x] = best;
  s_idx[threadIdx.x] = best_i;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d && sweep_better(s_phi[threadIdx.x + d], s_idx[threadIdx.x + d], s_phi[threadIdx.x], s_idx[threadIdx.x])) {
      s_phi[threadIdx.x] = s_phi[threadIdx.x + d];
      s_idx[threadIdx.x] = s_idx[threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const u64 bi = s_idx[0];
    const bool have = bi != ~0ull;
    hdr[1] = have ? bi + 1 : 0ull;
    hdr[2] = have ? cut[bi] : 0ull;
    hdr[3] = have ? volx[bi + 1] : 0ull;
    hdr[4] = (u64)__double_as_longlong(s_phi[0]);
    hdr[5] = volx[profiled];
  }
}

// ------------------------------------------------------------------ launchers
// PPRHIP_SWEEP_ITEM_GRID / PPRHIP_SWEEP_EDGE_GRID (test switches, read at every launch): at most so many workgroups, so
// that a graph of a few thousand nodes and a few tiles gives a workgroup a second and a third turn of its stride loop
static uint32_t sweep_grid_cap(const char* name, uint32_t grid) {
  if (const char* e = hook_env(name))
    if (atol(e) > 0) grid = (uint32_t)std::min<long>((long)grid, atol(e));
  return grid;
}

static uint32_t sweep_grid(uint64_t items, uint32_t cap) {
  const uint64_t b = (items + 255) / 256;
  return sweep_grid_cap("PPRHIP_SWEEP_ITEM_GRID", (uint32_t)(b < 1 ? 1 : (b > cap ? cap : b)));
}

// the two grids for the launchers of kernels_weighted_sweep.hip, which the same switches cap
uint32_t sweep_item_grid(uint64_t items, uint32_t cap) { return sweep_grid(items, cap); }
uint32_t sweep_edge_grid(uint32_t grid) { return sweep_grid_cap("PPRHIP_SWEEP_EDGE_GRID", grid); }

int launch_sweep_support(pprhip_graph* g, SweepWs* w, const double* x, int normalize) {
  const GraphData* D = g->gr;
  PPRHIP_CHECK_HIP(hipMemsetAsync(w->hdr, 0, sizeof(u64) * kSweepHdrWords, g->stream));
  hipLaunchKernelGGL(k_sweep_support, dim3(sweep_grid(D->n, 2048)), dim3(256), 0, g->stream, x, D->n, D->out_rp, D->in_rp,
                     D->new2old, normalize, w->key[0], w->id[0], w->hdr);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// the library calls' scratch: grown when a call asks for more than there is
static int sweep_tmp(SweepWs* w, size_t need) {
  if (need <= w->tmp_bytes) return PPRHIP_OK;
  if (w->tmp) (void)hipFree(w->tmp);  // (waits for the work queued on it)
  w->tmp = nullptr;
  w->tmp_bytes = 0;
  const hipError_t e = hipMalloc(&w->tmp, need);
  if (e != hipSuccess) {
    set_error("sweep: hipMalloc(%zu bytes) failed: %s", need, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? PPRHIP_ERR_OOM : PPRHIP_ERR_HIP;
  }
  w->tmp_bytes = need;
  return PPRHIP_OK;
}

// stable sorts, least significant criterion first: by original id, then by key; w->order names the sorted ids
int launch_sweep_sort(pprhip_graph* g, SweepWs* w, uint32_t count) {
  unsigned id_bits = 1;
  while (id_bits < 32 && (1ull << id_bits) < (u64)g->gr->n) ++id_bits;
  rocprim::double_buffer<uint32_t> di(w->id[0], w->id[1]);
  rocprim::double_buffer<u64> dk(w->key[0], w->key[1]);
  size_t b0 = 0, b1 = 0;
  if (rocprim::radix_sort_pairs(nullptr, b0, di, dk, (size_t)count, 0u, id_bits, g->stream) != hipSuccess ||
      rocprim::radix_sort_pairs(nullptr, b1, dk, di, (size_t)count, 0u, 63u, g->stream) != hipSuccess) {
    set_error("sweep: sizing the device sort failed");
    return PPRHIP_ERR_HIP;
  }
  PPRHIP_TRY(sweep_tmp(w, std::max<size_t>(std::max(b0, b1), 16)));
  size_t b = w->tmp_bytes;
  if (rocprim::radix_sort_pairs(w->tmp, b, di, dk, (size_t)count, 0u, id_bits, g->stream) != hipSuccess) {
    set_error("sweep: the device sort by id failed");
    return PPRHIP_ERR_HIP;
  }
  b = w->tmp_bytes;
  // (bit 63 of a key is the inverted sign of a positive score: set in every key)
  if (rocprim::radix_sort_pairs(w->tmp, b, dk, di, (size_t)count, 0u, 63u, g->stream) != hipSuccess) {
    set_error("sweep: the device sort by score failed");
    return PPRHIP_ERR_HIP;
  }
  w->order = di.current();
  return PPRHIP_OK;
}

int sweep_scan(pprhip_graph* g, SweepWs* w, const u64* in, u64* out, uint32_t count) {
  size_t b = 0;
  if (rocprim::inclusive_scan(nullptr, b, in, out, (size_t)count, rocprim::plus<u64>(), g->stream) != hipSuccess) {
    set_error("sweep: sizing the device scan failed");
    return PPRHIP_ERR_HIP;
  }
  PPRHIP_TRY(sweep_tmp(w, std::max<size_t>(b, 16)));
  b = w->tmp_bytes;
  if (rocprim::inclusive_scan(w->tmp, b, in, out, (size_t)count, rocprim::plus<u64>(), g->stream) != hipSuccess) {
    set_error("sweep: the device scan failed");
    return PPRHIP_ERR_HIP;
  }
  return PPRHIP_OK;
}

// rank[v] = position for the first `profiled` positions ("none" elsewhere), the positions' row extents, vol
int launch_sweep_rank(pprhip_graph* g, SweepWs* w, uint32_t profiled) {
  const GraphData* D = g->gr;
  PPRHIP_CHECK_HIP(hipMemsetAsync(w->rank, 0xFF, sizeof(uint32_t) * (size_t)D->n, g->stream));  // kSweepNone
  hipLaunchKernelGGL(k_sweep_rank, dim3(sweep_grid(profiled, 2048)), dim3(256), 0, g->stream, w->order, profiled,
                     D->old2new, D->out_rp, D->in_rp, w->rank, w->rec, w->deg, w->volx);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return sweep_scan(g, w, w->deg, w->volx + 1, profiled);
}

int launch_sweep_tile_starts(pprhip_graph* g, SweepWs* w, uint32_t profiled) {
  const uint64_t max_tiles = std::max<uint64_t>(1, (2 * g->gr->m + kSweepTile - 1) / kSweepTile);  // (<= w->tile_cap)
  hipLaunchKernelGGL(k_sweep_tile_starts, dim3(sweep_grid(max_tiles, 1024)), dim3(256), 0, g->stream, w->volx, profiled,
                     w->tile_node);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// delta over the slot space, then cut = its scan
int launch_sweep_edges(pprhip_graph* g, SweepWs* w, uint32_t profiled, hipEvent_t before, hipEvent_t after) {
  const GraphData* D = g->gr;
  const uint64_t max_tiles = std::max<uint64_t>(1, (2 * D->m + kSweepTile - 1) / kSweepTile);  // (<= w->tile_cap)
  PPRHIP_TRY(launch_sweep_tile_starts(g, w, profiled));
  PPRHIP_CHECK_HIP(hipEventRecord(before, g->stream));
  PPRHIP_CHECK_HIP(hipMemsetAsync(w->delta, 0, sizeof(long long) * (size_t)profiled, g->stream));
  // 32 KB of LDS per workgroup: five of them share a CU
  const uint32_t grid =
      sweep_grid_cap("PPRHIP_SWEEP_EDGE_GRID", (uint32_t)std::min<uint64_t>(max_tiles, (uint64_t)D->n_cus * 5u));
  hipLaunchKernelGGL(k_sweep_edges, dim3(grid), dim3(256), 0, g->stream, w->volx, profiled, w->tile_node, w->rec, w->rank,
                     D->out_ci, D->in_ci, w->delta);
  PPRHIP_CHECK_HIP(hipGetLastError());
  PPRHIP_CHECK_HIP(hipEventRecord(after, g->stream));
  return sweep_scan(g, w, reinterpret_cast<const u64*>(w->delta), w->cut, profiled);
}

int launch_sweep_best_over(pprhip_graph* g, SweepWs* w, const u64* volx, const u64* cut, uint32_t profiled,
                           uint64_t total_vol, uint64_t max_vol) {
  const uint32_t grid = sweep_grid(profiled, kSweepBestBlocks);
  hipLaunchKernelGGL(k_sweep_best, dim3(grid), dim3(256), 0, g->stream, volx, cut, profiled, (u64)total_vol, (u64)max_vol,
                     w->part_phi, w->part_idx);
  hipLaunchKernelGGL(k_sweep_best_final, dim3(1), dim3(256), 0, g->stream, w->part_phi, w->part_idx, grid, volx, cut,
                     profiled, w->hdr);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_sweep_best(pprhip_graph* g, SweepWs* w, uint32_t profiled, uint64_t max_vol) {
  return launch_sweep_best_over(g, w, w->volx, w->cut, profiled, 2ull * g->gr->m, max_vol);
}

int init_kernels_sweep() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_sweep_edges)));
  return PPRHIP_OK;
}

}  // namespace pprhip
