// kernels_weighted_query.hip — weighted seed sets and weighted top-k rounds for gfx950 (MI355X): what a weighted push
// needs beyond kernels_weighted.hip to start from a seed table, to land dead-end mass on p, and to be resumed at a
// lower threshold (DESIGN.md §2 "Weighted seed sets and top-k"; weighted_query.cpp drives them).
//
//   k_wq_land_sparse  between k_w_prepare and k_w_push of a sparse level: the level's dead-end mass x (ctr->dead) lands
//                     on p - r(i) += x q_i for every live seed with the push's crossing test, crossers appended to the
//                     next list; reserve(j) += x e_j for every dead-end seed - and the cell is cleared, so that
//                     k_w_push's own landing (which indexes out_ext[src], src = -1 here) sees it empty.
//   k_wq_land_dense   behind the seeded k_w_dense_apply (which gave the live seeds x w_node[u] inside their rows): the
//                     dead-end seeds' share, and the cell cleared.
//   k_wq_collect      a round's first frontier: the nodes active at the round's threshold, with the exclusive prefix of
//                     their out-degrees (k_w_push locates an edge by it) and the packed (count, edges) cell.
//
// The seed table is small beside a level (a few thousand entries at most: Neo4j's sourceNodes) and the landing is a
// read-modify-write per DISTINCT node, so both landing kernels are one workgroup: no atomics on the residues, and the
// cell is cleared behind a workgroup barrier instead of a grid-wide count.
#include "weighted_device.hpp"

namespace pprhip {

constexpr uint32_t kWqTile = 1024;  // nodes of k_wq_collect a workgroup compacts with one packed atomic

__global__ __launch_bounds__(256) void k_wq_land_sparse(const int32_t* __restrict__ id, const double* __restrict__ w,
                                                         uint32_t n_live, uint32_t n_all,
                                                         const unsigned long long* __restrict__ out_ext,
                                                         double* __restrict__ res, double* __restrict__ reserve,
                                                         int32_t* __restrict__ Fn, uint32_t* __restrict__ eoffn,
                                                         DevCounters* ctr, int dead_slot,
                                                         unsigned long long* out_counter, double rmax) {
  __shared__ WNewList s_new;
  const double x = ctr->dead[dead_slot];
  if (threadIdx.x == 0) s_new.count = 0;
  __syncthreads();  // (every thread holds x before the cell is cleared below)
  if (!(x > 0.0)) return;
  for (uint32_t base = 0; base < n_all; base += 256u) {  // (uniform trip count: w_flush_new holds barriers)
    const uint32_t i = base + threadIdx.x;
    if (i < n_live) {
      const int32_t u = id[i];
      const double add = x * w[i];
      const double old = res[u];  // a seed is listed once and nothing else runs: no atomic
      res[u] = old + add;
      w_push_finish(u, add, old, (uint32_t)(out_ext[u] >> 32), &s_new, rmax);
    } else if (i < n_all) {
      const int32_t u = id[i];
      reserve[u] = reserve[u] + x * w[i];
    }
    w_flush_new(&s_new, Fn, eoffn, out_counter);
  }
  if (threadIdx.x == 0) ctr->dead[dead_slot] = 0.0;
}

__global__ __launch_bounds__(256) void k_wq_land_dense(const int32_t* __restrict__ id, const double* __restrict__ w,
                                                        uint32_t n_live, uint32_t n_all, double* __restrict__ reserve,
                                                        DevCounters* ctr, int dead_slot) {
  const double x = ctr->dead[dead_slot];
  __syncthreads();
  if (!(x > 0.0)) return;
  for (uint32_t i = n_live + threadIdx.x; i < n_all; i += 256u) reserve[id[i]] = reserve[id[i]] + x * w[i];
  if (threadIdx.x == 0) ctr->dead[dead_slot] = 0.0;
}

// A workgroup owns whole tiles of kWqTile consecutive nodes, `tiles_per` of them in a row; inside its range the list is
// in id order with the running degree prefix (block_range_compact), ranges are placed in the order their one packed
// atomic arrives.  *counter is zero before and holds entries << 36 | edges after.
__global__ __launch_bounds__(256) void k_wq_collect(uint32_t n, uint32_t tiles_per, const double* __restrict__ res,
                                                     const unsigned long long* __restrict__ out_ext,
                                                     int32_t* __restrict__ F, uint32_t* __restrict__ eoff,
                                                     unsigned long long* counter, double rmax) {
  const unsigned long long span = (unsigned long long)tiles_per * kWqTile;
  const unsigned long long lo64 = (unsigned long long)blockIdx.x * span;
  if (lo64 >= n) return;
  const uint32_t lo = (uint32_t)lo64;
  const uint32_t hi = lo64 + span < n ? (uint32_t)(lo64 + span) : n;
  block_range_compact(
      lo, hi, counter,
      [&](uint32_t v, unsigned long long* wgt) {
        const uint32_t d = (uint32_t)(out_ext[v] >> 32);
        if (!active_fwd(res[v], d, rmax)) return false;
        *wgt = d;
        return true;
      },
      [&](uint32_t v, uint32_t pos, unsigned long long eo, unsigned long long) {
        F[pos] = (int32_t)v;
        eoff[pos] = (uint32_t)eo;
      });
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
int launch_wq_land_sparse(pprhip_graph* g, const PushArgs& a, int fbuf, int dead_slot, unsigned long long* next_counter) {
  const SeedTable* sd = g->seeds;
  k_wq_land_sparse<<<dim3(1), dim3(256), 0, g->stream>>>(sd->id, sd->w, sd->n_live, sd->n_live + sd->n_dead, g->gr->out_ext,
                                                         g->residue, g->reserve, g->F[fbuf ^ 1], g->eoff[fbuf ^ 1], g->ctr,
                                                         dead_slot, next_counter, a.rmax);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_wq_land_dense(pprhip_graph* g, int dead_slot) {
  const SeedTable* sd = g->seeds;
  k_wq_land_dense<<<dim3(1), dim3(256), 0, g->stream>>>(sd->id, sd->w, sd->n_live, sd->n_live + sd->n_dead, g->reserve,
                                                        g->ctr, dead_slot);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_wq_collect(pprhip_graph* g, double rmax, int out_fbuf, unsigned long long* d_counter) {
  const uint32_t n = act_n(g);
  const uint32_t tiles = (n + kWqTile - 1) / kWqTile;
  const uint32_t grid = std::max(1u, std::min(tiles, 16384u));
  const uint32_t tiles_per = std::max(1u, (tiles + grid - 1) / grid);
  k_wq_collect<<<dim3(grid), dim3(256), 0, g->stream>>>(n, tiles_per, g->residue, g->gr->out_ext, g->F[out_fbuf],
                                                        g->eoff[out_fbuf], d_counter, rmax);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int init_kernels_weighted_query() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_wq_collect)));
  return PPRHIP_OK;
}

}  // namespace pprhip
