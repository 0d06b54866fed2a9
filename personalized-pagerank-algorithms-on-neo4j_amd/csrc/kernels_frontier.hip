// kernels_frontier.hip — the passes that start a query or change a level's shape, and the small reductions and copies
// around them, for gfx950 (MI355X).  The levels themselves: kernels_push.hip, kernels_dense.hip.
#include "push_device.hpp"

namespace pprhip {

// ------------------------------------------------------------------------------------------------
// frontier seeding (round starts) and conversions between the two level shapes
// ------------------------------------------------------------------------------------------------
// seed kinds: 0 = every node that meets the (new) threshold (a FORA round after a halving);
//             1 = top-k round start from the parked set (Forward_Push.java:163,173,241-247)
template <int KIND>
__device__ __forceinline__ bool seed_pred(uint32_t v, const double* __restrict__ res, uint32_t d,
                                          const uint8_t* __restrict__ flags, const PushArgs& a) {
  if (KIND == 1 && !flags[v]) return false;
  return active_fwd(res[v], d, a.rmax);
}

// top-k round start: parked nodes that start the round leave the parked set; parked nodes that
// fell below min_rmax are dropped (Forward_Push.java:241-247 keeps the others parked)
__device__ __forceinline__ void unpark(uint32_t v, const double* __restrict__ res, uint32_t d,
                                       uint8_t* __restrict__ flags, const PushArgs& a) {
  if (!flags[v]) return;
  const double r = res[v];
  if (active_fwd(r, d, a.rmax) || !active_fwd(r, d, a.min_rmax)) flags[v] = 0;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_count_active(uint32_t n, const double* __restrict__ res,
                                                       const uint32_t* __restrict__ out_rp,
                                                       const uint8_t* __restrict__ flags, uint32_t* __restrict__ armed,
                                                       unsigned long long* __restrict__ blk_pack,
                                                       unsigned long long* zero_word, PushArgs a) {
  __shared__ unsigned long long s_red2[4];
  unsigned long long pack = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0ull;  // the list counter of the seeding pass that follows
  // wave-uniform trip count: a wave covers 64 consecutive nodes, whose "armed" bits it writes as one 64-bit word
  for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += gridDim.x * blockDim.x) {
    const uint32_t v = base + (threadIdx.x & 63u);
    bool arm = false;
    if (v < n) {
      const uint32_t d = out_rp[v + 1] - out_rp[v];
      if (seed_pred<KIND>(v, res, d, flags, a)) pack += (1ull << kPackShift) | (unsigned long long)d;
      // top-k rounds: meets the round's threshold without being parked (only when rmax < min_rmax)
      if (KIND == 1) arm = a.rmax < a.min_rmax && !flags[v] && active_fwd(res[v], d, a.rmax);
    }
    if (KIND == 1) {
      const unsigned long long bits = __ballot(arm);
      if ((threadIdx.x & 63u) == 0) {
        armed[base >> 5] = (uint32_t)bits;
        armed[(base >> 5) + 1] = (uint32_t)(bits >> 32);
      }
    }
  }
  const unsigned long long ps = block_sum_u64(pack, s_red2);
  if (threadIdx.x == 0) blk_pack[blockIdx.x] = ps;
}

// `armed` (top-k round starts that do not count first): the pass also writes the round's "armed" bits, as
// k_count_active does; the workgroups' ranges are multiples of 256 nodes then, so a wave covers 64 consecutive ids.
template <int KIND>
__global__ __launch_bounds__(256) void k_seed_list(uint32_t n, const double* __restrict__ res,
                                                    const uint32_t* __restrict__ out_rp, uint8_t* __restrict__ flags,
                                                    int32_t* __restrict__ Fn, uint32_t* __restrict__ eoffn,
                                                    unsigned long long* counter, uint32_t* __restrict__ armed, PushArgs a) {
  uint32_t per = (n + gridDim.x - 1) / gridDim.x;
  if (armed) per = (per + 255u) & ~255u;
  const unsigned long long lo64 = (unsigned long long)blockIdx.x * per;
  if (lo64 >= n) return;
  const uint32_t lo = (uint32_t)lo64;
  const uint32_t hi = lo64 + per < n ? lo + per : n;
  block_range_compact(
      lo, hi, counter,
      [&](uint32_t v, unsigned long long* w) {
        const uint32_t d = out_rp[v + 1] - out_rp[v];
        *w = d;
        return seed_pred<KIND>(v, res, d, flags, a);
      },
      [&](uint32_t v, uint32_t pos, unsigned long long eo, unsigned long long) {
        Fn[pos] = (int32_t)v;
        eoffn[pos] = (uint32_t)eo;
      });
  if (KIND == 1) {
    __syncthreads();
    // wave-uniform trip count: a wave covers 64 consecutive nodes, whose "armed" bits it writes as one 64-bit word
    for (uint32_t base = lo + (threadIdx.x & ~63u); base < hi; base += 256) {
      const uint32_t v = base + (threadIdx.x & 63u);
      bool arm = false;
      if (v < hi) {
        const uint32_t d = out_rp[v + 1] - out_rp[v];
        // meets the round's threshold without being parked (only when rmax < min_rmax); tested before the node leaves
        // the parked set
        if (armed) arm = a.rmax < a.min_rmax && !flags[v] && active_fwd(res[v], d, a.rmax);
        unpark(v, res, d, flags, a);
      }
      if (armed) {
        const unsigned long long bits = __ballot(arm);
        if ((threadIdx.x & 63u) == 0) {
          armed[base >> 5] = (uint32_t)bits;
          armed[(base >> 5) + 1] = (uint32_t)(bits >> 32);
        }
      }
    }
  }
}

// k_seed_list<1> in one pass (round 5): a workgroup takes tiles of 2048 consecutive nodes, a thread 8 consecutive ones -
// its flags are one 8-byte load, its residues four 16-byte loads, its row pointers three - lists the round's start set
// (block_tile_compact), writes the armed bits of its 8 nodes as one byte and lets the parked nodes go with one 8-byte
// store.  Same list order (ascending ids), same bits, same flags as the two-pass kernel; 41 -> ~10 us on R-MAT 22.
constexpr int kSeedItems = 8;
__global__ __launch_bounds__(256) void k_seed_list_topk(uint32_t n, const double* __restrict__ res,
                                                         const uint32_t* __restrict__ out_rp, uint8_t* __restrict__ flags,
                                                         int32_t* __restrict__ Fn, uint32_t* __restrict__ eoffn,
                                                         unsigned long long* counter, uint32_t* __restrict__ armed, PushArgs a) {
  const uint32_t tile = 256u * kSeedItems;
  const uint32_t n_tiles = (n + tile - 1) / tile;
  for (uint32_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const uint32_t v0 = tl * tile + threadIdx.x * kSeedItems;
    bool take[kSeedItems];
    unsigned long long w[kSeedItems];
    double r[kSeedItems];
    uint32_t deg[kSeedItems];
    uint8_t fl[kSeedItems];
    if (v0 + kSeedItems <= n) {  // (n + 1 row pointers and n flags exist: whole groups of 8 load as vectors)
      const unsigned long long f8 = *reinterpret_cast<const unsigned long long*>(flags + v0);
#pragma unroll
      for (int i = 0; i < kSeedItems; ++i) fl[i] = (uint8_t)(f8 >> (8 * i));
      const double2* r2 = reinterpret_cast<const double2*>(res + v0);
#pragma unroll
      for (int i = 0; i < kSeedItems / 2; ++i) {
        const double2 x = r2[i];
        r[2 * i] = x.x;
        r[2 * i + 1] = x.y;
      }
      const uint4* p4 = reinterpret_cast<const uint4*>(out_rp + v0);  // (v0 is a multiple of 8: 32-byte aligned)
      const uint4 x0 = p4[0], x1 = p4[1];
      const uint32_t last = out_rp[v0 + 8];
      deg[0] = x0.y - x0.x; deg[1] = x0.z - x0.y; deg[2] = x0.w - x0.z; deg[3] = x1.x - x0.w;
      deg[4] = x1.y - x1.x; deg[5] = x1.z - x1.y; deg[6] = x1.w - x1.z; deg[7] = last - x1.w;
    } else {
#pragma unroll
      for (int i = 0; i < kSeedItems; ++i) {
        const bool in = v0 + i < n;
        fl[i] = in ? flags[v0 + i] : 0;
        r[i] = in ? res[v0 + i] : 0.0;
        deg[i] = in ? out_rp[v0 + i + 1] - out_rp[v0 + i] : 0u;
      }
    }
    uint32_t arm_bits = 0;
    unsigned long long f_new = 0;
#pragma unroll
    for (int i = 0; i < kSeedItems; ++i) {
      const uint32_t d = deg[i];
      const bool in = v0 + i < n;
      const bool act = in && active_fwd(r[i], d, a.rmax);
      take[i] = act && fl[i];  // seed_pred<1>
      w[i] = d;
      // meets the round's threshold without being parked (only when rmax < min_rmax): tested before the node leaves the set
      if (a.rmax < a.min_rmax && !fl[i] && act) arm_bits |= 1u << i;
      // unpark: parked nodes that start the round leave the set; those below min_rmax are dropped
      uint8_t f = fl[i];
      if (f && (act || !active_fwd(r[i], d, a.min_rmax))) f = 0;
      f_new |= (unsigned long long)f << (8 * i);
    }
    block_tile_compact<kSeedItems>(take, w, counter, [&](int i, uint32_t pos, unsigned long long eo) {
      Fn[pos] = (int32_t)(v0 + i);
      eoffn[pos] = (uint32_t)eo;
    });
    if (v0 < n) {
      if (armed) reinterpret_cast<uint8_t*>(armed)[v0 >> 3] = (uint8_t)arm_bits;
      if (v0 + kSeedItems <= n) {
        *reinterpret_cast<unsigned long long*>(flags + v0) = f_new;
      } else {
#pragma unroll
        for (int i = 0; i < kSeedItems; ++i)
          if (v0 + i < n) flags[v0 + i] = (uint8_t)(f_new >> (8 * i));
      }
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_seed_dense(uint32_t n, double* __restrict__ res, double* __restrict__ reserve,
                                                     const uint32_t* __restrict__ out_rp, uint8_t* __restrict__ flags,
                                                     CView c_dense, unsigned long long* __restrict__ blk_pack,
                                                     double* __restrict__ blk_dead, uint32_t* __restrict__ blk_ndead,
                                                     PushArgs a) {
  __shared__ double s_red[4];
  __shared__ unsigned long long s_red2[4];
  double dead = 0.0;
  unsigned long long pack = 0, ndead = 0;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint32_t d = out_rp[v + 1] - out_rp[v];
    double c = 0.0;
    const bool take = seed_pred<KIND>(v, res, d, flags, a);
    if (KIND == 1) unpark(v, res, d, flags, a);
    if (take) {
      const double rc = res[v];
      res[v] = 0.0;
      reserve[v] = reserve[v] + rc * a.alpha;
      if (d == 0) {
        dead += rc * (1.0 - a.alpha);
        ndead++;
      } else {
        c = ((1.0 - a.alpha) * rc) / (double)d;
      }
      pack += (1ull << kPackShift) | (unsigned long long)d;
    }
    if (c_dense.stride == 1 || c != 0.0) c_dense.at(v) = c;  // a slot's column is all-zero beforehand
  }
  const double ds = block_sum_f64(dead, s_red);
  const unsigned long long ps = block_sum_u64(pack, s_red2);
  const unsigned long long nd = block_sum_u64(ndead, s_red2);
  if (threadIdx.x == 0) {
    blk_pack[blockIdx.x] = ps;
    blk_dead[blockIdx.x] = ds;
    blk_ndead[blockIdx.x] = (uint32_t)nd;
  }
}

// dense-prepared state -> sparse-prepared state: list every node holding a contribution
__global__ __launch_bounds__(256) void k_compact_prepared(uint32_t n, CView c_dense, bool clear,
                                                           const uint32_t* __restrict__ trp, int32_t* __restrict__ Fn,
                                                           uint32_t* __restrict__ eoffn, double* __restrict__ cF,
                                                           unsigned long long* counter) {
  const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
  const uint32_t lo = blockIdx.x * per;
  const uint32_t hi = lo + per < n ? lo + per : n;
  if (lo >= hi) return;
  block_range_compact(
      lo, hi, counter,
      [&](uint32_t v, unsigned long long* w) {
        if (!(c_dense.at(v) > 0.0)) return false;
        *w = trp[v + 1] - trp[v];
        return true;
      },
      [&](uint32_t v, uint32_t pos, unsigned long long eo, unsigned long long) {
        Fn[pos] = (int32_t)v;
        eoffn[pos] = (uint32_t)eo;
        cF[pos] = c_dense.at(v);
        if (clear) c_dense.at(v) = 0.0;  // a slot leaving the dense shape hands back an all-zero column
      });
}

// the same for a batch slot after a sweep: the apply kernel left one bit per row ordinal that holds a
// contribution, so only those entries of the slot's column are read (and handed back as zero)
__global__ __launch_bounds__(256) void k_compact_bits(uint32_t n_rows, uint32_t n_nz,
                                                       const unsigned long long* __restrict__ bits,
                                                       const int32_t* __restrict__ nz_rows,
                                                       const int32_t* __restrict__ zin_rows, CView c_dense,
                                                       const uint32_t* __restrict__ trp, int32_t* __restrict__ Fn,
                                                       uint32_t* __restrict__ eoffn, double* __restrict__ cF,
                                                       unsigned long long* counter) {
  const uint32_t per = (((n_rows + gridDim.x - 1) / gridDim.x) + 63u) & ~63u;
  const uint32_t lo = blockIdx.x * per;
  const uint32_t hi = lo + per < n_rows ? lo + per : n_rows;
  if (lo >= hi) return;
  block_range_compact(
      lo, hi, counter,
      [&](uint32_t j, unsigned long long* w) {
        if (!((bits[j >> 6] >> (j & 63)) & 1ull)) return false;
        const int32_t u = j < n_nz ? nz_rows[j] : zin_rows[j - n_nz];
        *w = trp[u + 1] - trp[u];
        return true;
      },
      [&](uint32_t j, uint32_t pos, unsigned long long eo, unsigned long long) {
        const int32_t u = j < n_nz ? nz_rows[j] : zin_rows[j - n_nz];
        Fn[pos] = u;
        eoffn[pos] = (uint32_t)eo;
        cF[pos] = c_dense.at((uint32_t)u);
        c_dense.at((uint32_t)u) = 0.0;
      });
}

// ------------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sum_partial(const double* __restrict__ x, uint32_t n,
                                                      double* __restrict__ partial) {
  __shared__ double s_red[4];
  double acc = 0.0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) acc += x[i];
  const double s = block_sum_f64(acc, s_red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_sum_final(const double* __restrict__ partial, uint32_t np, DevCounters* ctr) {
  __shared__ double s_red[4];
  double acc = 0.0;
  for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) acc += partial[i];
  const double s = block_sum_f64(acc, s_red);
  if (threadIdx.x == 0) ctr->sum_out = s;
}

__global__ void k_set_f64(double* p, uint32_t idx, double value) { p[idx] = value; }

__global__ __launch_bounds__(256) void k_permute_out(const double* __restrict__ x, const int32_t* __restrict__ old2new,
                                                      double* __restrict__ out, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = x[old2new[i]];
}

// ------------------------------------------------------------------------------------------------
// seed sets (engine.hpp: SeedTable): a query personalized to a weighted node set p
// ------------------------------------------------------------------------------------------------
// Query start: r = q on the live seeds, reserve = e on the dead-end seeds (p resolved once, as if mass 1 landed on it),
// the live seeds' landing weights per node, and the live seeds as the first frontier list (edge offsets from the host)
// - or, top-k (flags != nullptr), as the parked set the first round starts from (Fora_Topk.java:117-118 for one seed).
__global__ __launch_bounds__(256) void k_seed_init(const int32_t* __restrict__ id, const double* __restrict__ w,
                                                    const uint32_t* __restrict__ eoff_in, uint32_t n_live, uint32_t n_all,
                                                    double* __restrict__ res, double* __restrict__ reserve,
                                                    double* __restrict__ w_node, int32_t* __restrict__ F,
                                                    uint32_t* __restrict__ eoff, uint8_t* __restrict__ flags) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += gridDim.x * blockDim.x) {
    const int32_t u = id[i];
    const double x = w[i];
    if (i < n_live) {
      res[u] = x;
      w_node[u] = x;
      if (flags) {
        flags[u] = 1;
      } else {
        F[i] = u;
        eoff[i] = eoff_in[i];
      }
    } else {
      reserve[u] = x;
    }
  }
}

// The landing weights of the set before go back to zero (the first `count` entries of its table: its live seeds).
__global__ __launch_bounds__(256) void k_seed_clear(const int32_t* __restrict__ id, uint32_t count,
                                                     double* __restrict__ w_node) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) w_node[id[i]] = 0.0;
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
int launch_compact_prepared(pprhip_graph* g, int cbuf, int out_fbuf, unsigned long long* d_counter, bool backward) {
  const uint32_t grid = grid_for(g->gr->n, 1024, 1024);
  const SweepSide S = sweep_side(g->gr, backward);
  if (g->parent) {
    // the rows the batched sweep carries (launch_dense_level_b8): one bit each, per slot, in tiles of kTileRows
    const uint32_t n_rows = S.n_nz + S.n_z;
    const uint32_t n_tiles = (n_rows + kTileRows - 1) / kTileRows;
    k_compact_bits<<<dim3(grid), dim3(256), 0, g->stream>>>(
        n_rows, S.n_nz, g->parent->batch->prep_bits + (size_t)g->slot_index * n_tiles, S.nz_rows, S.z_rows, cview(g, cbuf),
        S.rp, g->F[out_fbuf], g->eoff[out_fbuf], g->cF, d_counter);
  } else {
    k_compact_prepared<<<dim3(grid), dim3(256), 0, g->stream>>>(act_n(g), cview(g, cbuf), false, S.rp, g->F[out_fbuf],
                                                                g->eoff[out_fbuf], g->cF, d_counter);
  }
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_count_active(pprhip_graph* g, const PushArgs& a, int seed_kind, int out_slot) {
  const uint32_t grid = grid_for(act_n(g), 256 * 8, 1024);
  const auto count = seed_kind == 0 ? &k_count_active<0> : &k_count_active<1>;
  count<<<dim3(grid), dim3(256), 0, g->stream>>>(act_n(g), g->residue, g->gr->out_rp, g->flags, g->armed, g->blk_pack,
                                                 &g->ctr->hist[kMaxBatch + 2], a);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return reduce_partials(g, grid, out_slot, 0, false);
}

bool old_small_kernels() {  // PPRHIP_TOPK_OLD_PASSES=1 (measurement switch): the two-pass kernels of rounds 1-4
  static const bool v = hook_env("PPRHIP_TOPK_OLD_PASSES") != nullptr;
  return v;
}

int launch_seed_list(pprhip_graph* g, const PushArgs& a, int seed_kind, int out_fbuf, unsigned long long* d_counter,
                     bool write_armed) {
  // 1024 nodes per workgroup (fewer or more were slower); a slot of a threaded batch keeps the cap of 1024
  // workgroups: with sixteen queries on the chip, smaller launches do better (1 018 vs 946-977 queries/s)
  const uint32_t grid = grid_for(act_n(g), 1024, g->sync ? 1024 : 16384);
  if (seed_kind == 0)
    k_seed_list<0><<<dim3(grid), dim3(256), 0, g->stream>>>(act_n(g), g->residue, g->gr->out_rp, g->flags, g->F[out_fbuf],
                                                            g->eoff[out_fbuf], d_counter, nullptr, a);
  else if (write_armed && !old_small_kernels()) {
    // (the one-pass form always rewrites the flags and the armed bits of every node: the round-start call)
    const uint32_t tiles = (act_n(g) + 256u * kSeedItems - 1) / (256u * kSeedItems);
    k_seed_list_topk<<<dim3(std::max(1u, tiles)), dim3(256), 0, g->stream>>>(act_n(g), g->residue, g->gr->out_rp, g->flags,
                                                                            g->F[out_fbuf], g->eoff[out_fbuf], d_counter,
                                                                            g->armed, a);
  } else
    k_seed_list<1><<<dim3(grid), dim3(256), 0, g->stream>>>(act_n(g), g->residue, g->gr->out_rp, g->flags, g->F[out_fbuf],
                                                            g->eoff[out_fbuf], d_counter, write_armed ? g->armed : nullptr, a);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_seed_dense(pprhip_graph* g, const PushArgs& a, int seed_kind, int cbuf, int out_slot, int dead_slot) {
  const uint32_t grid = grid_for(act_n(g), 256 * 8, 1024);
  const auto seed = seed_kind == 0 ? &k_seed_dense<0> : &k_seed_dense<1>;
  seed<<<dim3(grid), dim3(256), 0, g->stream>>>(act_n(g), g->residue, g->reserve, g->gr->out_rp, g->flags, cview(g, cbuf),
                                                g->blk_pack, g->blk_dead, g->blk_ndead, a);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return reduce_partials(g, grid, out_slot, dead_slot, true);
}

int launch_sum(pprhip_graph* g, const double* x, uint32_t n) {
  const uint32_t np = grid_for(n, 256 * 16, 1024);
  k_sum_partial<<<dim3(np), dim3(256), 0, g->stream>>>(x, n, g->partial);
  k_sum_final<<<dim3(1), dim3(256), 0, g->stream>>>(g->partial, np, g->ctr);
  PPRHIP_CHECK_HIP(hipGetLastError());
  g->sum_np = 0;
  return PPRHIP_OK;
}

// the partial sums only: the walk plan that follows (launch_mc_plan with the budget derived on the device) adds them up
// itself, in every workgroup - one launch less on the chain of a top-k round
int launch_sum_partial(pprhip_graph* g, const double* x, uint32_t n) {
  if (old_small_kernels()) return launch_sum(g, x, n);
  const uint32_t np = grid_for(n, 256 * 8, 1024);
  k_sum_partial<<<dim3(np), dim3(256), 0, g->stream>>>(x, n, g->partial);
  PPRHIP_CHECK_HIP(hipGetLastError());
  g->sum_np = np;
  return PPRHIP_OK;
}

int launch_permute_out(pprhip_graph* g, const double* x, double* out) {
  k_permute_out<<<dim3(grid_for(g->gr->n, 256, 4096)), dim3(256), 0, g->stream>>>(x, g->gr->old2new, out, g->gr->n);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_set_f64(pprhip_graph* g, double* p, uint32_t idx, double value) {
  k_set_f64<<<dim3(1), dim3(1), 0, g->stream>>>(p, idx, value);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_seed_init(pprhip_graph* g, int fbuf, bool topk) {
  const SeedTable* sd = g->seeds;
  const uint32_t n_all = sd->n_live + sd->n_dead;
  k_seed_init<<<dim3(grid_for(n_all, 256, 4096)), dim3(256), 0, g->stream>>>(
      sd->id, sd->w, sd->eoff, sd->n_live, n_all, g->residue, g->reserve, sd->w_node, g->F[fbuf], g->eoff[fbuf],
      topk ? g->flags : nullptr);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_seed_clear(pprhip_graph* g, uint32_t count) {
  if (!count) return PPRHIP_OK;
  const SeedTable* sd = g->seeds;
  k_seed_clear<<<dim3(grid_for(count, 256, 4096)), dim3(256), 0, g->stream>>>(sd->id, count, sd->w_node);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int init_kernels_frontier() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_count_active<0>)));
  return PPRHIP_OK;
}

}  // namespace pprhip
