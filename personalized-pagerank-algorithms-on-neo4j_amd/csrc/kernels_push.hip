// kernels_push.hip — the sparse frontier level for gfx950 (MI355X).
//
// One *level* pushes every frontier node at once from its residue at level start (the frontier-synchronous form of
// Forward_Push.java:86-139 / Backward_Search.java:58-96).  A level runs in one of two shapes: sparse (this file) or
// dense (kernels_dense.hip; sixteen queries per sweep: kernels_dense_batch.hip).  The passes that start a query or
// change a level's shape are in kernels_frontier.hip, what the four files share in push_device.hpp.
//
//   sparse  k_sparse_prepare (per frontier node: take the residue, credit the reserve, compute the
//           per-edge contribution) then k_sparse_push (edge-parallel over the frontier's edges:
//           frontier entries staged in LDS, coalesced col_idx reads, one returning fp64 atomic per
//           edge, threshold-crossing detection on (old, old + c), crossings collected in LDS and
//           appended to the next frontier with one packed atomic per 2048-edge tile).  Sparse
//           levels are launched in batches: every level's (nodes, edges) counter lives in a small
//           device-side history, and a level's kernels return at once when the previous level left
//           nothing to do (or left so much that the host should switch to the dense shape), so the
//           host reads counters back once per batch, not once per level.
//           (Round 4 tried the batch as ONE launch - prepare and push of up to eight levels inside a kernel whose
//           workgroups meet at a barrier between the steps, shared state read and written past the L2s - and took it
//           back: with grids of 1 to 128 workgroups it was slower everywhere, 2.11-2.23 ms per top-k query against
//           2.04, 0.39-0.55 ms of sparse levels per headline query against 0.34 (profiles/r04_sparse_levels_study.txt).
//           Launches queued back to back overlap their own overhead, and a gated launch costs 3 us; a barrier of
//           memory-side atomics and levels run by fewer workgroups cost more.)
//
// HBM-bound integer/fp64 work: no MFMA anywhere.  All arithmetic is IEEE double with
// -ffp-contract=off so each product / quotient rounds exactly as the reference's Java does.
#include "push_device.hpp"

namespace pprhip {

constexpr int kPushTile = 2048;  // edges per workgroup iteration of k_sparse_push
constexpr int kStageCap = 512;   // frontier entries staged in LDS at a time
constexpr int kCombSlots = 2048;     // LDS table that sums a tile's contributions per destination (power of two)
constexpr int kCombProbes = 4;       // slots tried before an edge goes to memory on its own
constexpr int kCombMinEdges = 262144;  // levels below this many edges skip the table (no gain measured there)

// A batched sparse level runs iff the level before it produced a non-empty frontier that is still
// worth running sparse (the host took that decision itself for the first level of a batch).
__device__ __forceinline__ bool level_runs(unsigned long long pk, int level, unsigned long long dense_thresh) {
  // The first level of a batch always runs: its list can be empty when it was compacted out of a
  // dense level that prepared dead-end nodes only, and their mass still has to land on the source.
  if (level == 0) return true;
  const unsigned long long nf = pk >> kPackShift, ef = pk & kPackMask;
  if (nf == 0) return false;
  return (nf + ef) < dense_thresh;
}

// ------------------------------------------------------------------------------------------------
// sparse level, step 1: every frontier node gives up its residue
// ------------------------------------------------------------------------------------------------
// (the body of k_sparse_prepare for workgroup `bid` of `nblk`: the one-workgroup kernel that runs several small levels
// in one launch, k_sparse_levels_wg, calls it with 0 of 1; pk: the level's frontier, entries << 36 | edges)
template <int MODE>
__device__ __forceinline__ void sparse_prepare_body(const int32_t* __restrict__ F, const uint32_t* __restrict__ out_rp,
                                                    double* __restrict__ res, double* __restrict__ reserve,
                                                    double* __restrict__ cF, CView c_dense, DevCounters* ctr, int level,
                                                    int dead_slot, unsigned long long pk0, unsigned long long pk,
                                                    const PushArgs& a, uint32_t bid, uint32_t nblk) {
  __shared__ double s_red[4];
  __shared__ unsigned long long s_red2[4];
  // the first level of a batch gets its frontier from the host as an argument (pk0 != ~0) and clears the counters of
  // the levels behind it: no copy and no fill on the stream for what two words and eight zeros say
  if (level == 0 && pk0 != ~0ull && bid == 0 && threadIdx.x == 0) {
    for (int i = 1; i <= kMaxBatch; ++i) ctr->hist[i] = 0ull;
    ctr->hist[kMaxBatch + 2] = 0ull;  // the seeding pass's list counter: the host has read it before this level
  }
  const uint32_t nf = (uint32_t)(pk >> kPackShift);
  double dead = 0.0;
  unsigned long long ndead = 0;
  for (uint32_t i = bid * blockDim.x + threadIdx.x; i < nf; i += nblk * blockDim.x) {
    const int32_t v = F[i];
    const double rc = res[v];
    res[v] = 0.0;                            // Forward_Push.java:89
    reserve[v] = reserve[v] + rc * a.alpha;  // :91-95
    double c;
    if (MODE == kBackward) {
      c = (1.0 - a.alpha) * rc;  // Backward_Search.java:72 (divided by d_out(u) per edge)
    } else {
      const uint32_t d = out_rp[v + 1] - out_rp[v];
      if (d == 0) {  // Forward_Push.java:101-104: the mass goes back to the source
        c = 0.0;
        dead += rc * (1.0 - a.alpha);
        ndead++;
      } else {
        c = ((1.0 - a.alpha) * rc) / (double)d;  // :117
      }
    }
    if (c_dense.p)
      c_dense.at((uint32_t)v) = c;
    else
      cF[i] = c;
  }
  if (MODE != kBackward) {
    const double ds = block_sum_f64(dead, s_red);
    const unsigned long long nd = block_sum_u64(ndead, s_red2);
    if (threadIdx.x == 0 && nd) {
      atomic_add_noret(&ctr->dead[dead_slot], ds);
      atomic_add_u64(&ctr->dead_pops, nd);
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_sparse_prepare(const int32_t* __restrict__ F,
                                                         const uint32_t* __restrict__ out_rp,
                                                         double* __restrict__ res, double* __restrict__ reserve,
                                                         double* __restrict__ cF, CView c_dense,
                                                         DevCounters* ctr, int level, unsigned long long dense_thresh,
                                                         int dead_slot, unsigned long long pk0, PushArgs a) {
  const unsigned long long pk = (level == 0 && pk0 != ~0ull) ? pk0 : ctr->hist[level];
  if (!level_runs(pk, level, dense_thresh)) {
    // (the counters behind a first level that does not run - it always runs - need no clearing)
    return;
  }
  sparse_prepare_body<MODE>(F, out_rp, res, reserve, cF, c_dense, ctr, level, dead_slot, pk0, pk, a, blockIdx.x, gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// sparse level, step 2: contributions land edge by edge
// ------------------------------------------------------------------------------------------------
struct NewList {  // crossings of the current tile, collected in LDS
  int32_t node[kPushTile + 1];
  uint32_t deg[kPushTile + 1];
  uint32_t count;
};

// One edge lands in three steps so that a thread can keep several edges in flight: the degree
// gather and the returning atomic are issued for a batch of edges before any result is used.
template <int MODE>
__device__ __forceinline__ void push_finish(int32_t u, double add, double old, uint32_t du,
                                            const uint32_t* __restrict__ in_rp, uint8_t* __restrict__ flags,
                                            uint32_t* __restrict__ armed, NewList* nl, const PushArgs& a) {
  const double nw = old + add;
  bool crossing;
  uint32_t adeg;
  if (MODE == kBackward) {
    crossing = !(old > a.rmax) && (nw > a.rmax);  // Backward_Search.java:89 strict, un-normalised
    adeg = crossing ? in_rp[u + 1] - in_rp[u] : 0u;
  } else {
    const bool was = active_fwd(old, du, a.rmax);
    crossing = !was && active_fwd(nw, du, a.rmax);  // Forward_Push.java:132
    adeg = du;
    if (MODE == kFwdTopk) {
      if (was && a.rmax < a.min_rmax) crossing = take_armed(armed, u);
      if (active_fwd(nw, du, a.min_rmax)) flags[u] = 1;  // :232-237 (parked)
    }
  }
  if (crossing) {
    const uint32_t slot = atomicAdd(&nl->count, 1u);
    nl->node[slot] = u;
    nl->deg[slot] = adeg;
  }
}

template <int MODE>
__device__ __forceinline__ void push_one(int32_t u, double c, const unsigned long long* __restrict__ out_ext,
                                         const uint32_t* __restrict__ in_rp, double* __restrict__ res,
                                         uint8_t* __restrict__ flags, uint32_t* __restrict__ armed, NewList* nl,
                                         const PushArgs& a) {
  const uint32_t du = (uint32_t)(out_ext[u] >> 32);  // packed row extent: one gather for the degree
  const double add = (MODE == kBackward) ? c / (double)du : c;  // Backward_Search.java:84-85
  const double old = atomic_add_ret(&res[u], add);               // Forward_Push.java:123-127
  push_finish<MODE>(u, add, old, du, in_rp, flags, armed, nl, a);
}

// Adds one edge's contribution to its destination's slot of the tile's LDS table (open addressing, a few probes);
// false when no slot could be had, and the edge then lands on its own.
__device__ __forceinline__ bool comb_insert(int32_t* s_key, double* s_val, int32_t u, double add) {
  uint32_t h = ((uint32_t)u * 2654435761u) >> (32 - 11);
  static_assert(kCombSlots == (1 << 11), "hash width follows the table size");
#pragma unroll
  for (int p = 0; p < kCombProbes; ++p) {
    int32_t k = s_key[h];
    if (k == -1) k = atomicCAS(&s_key[h], -1, u);
    if (k == -1 || k == u) {
      __hip_atomic_fetch_add(&s_val[h], add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return true;
    }
    h = (h + 1) & (kCombSlots - 1);
  }
  return false;
}

// Appends the tile's crossings to the next frontier: one packed atomic reserves list slots and
// the edge range, a workgroup scan turns the degrees into edge offsets.
__device__ __forceinline__ void flush_new(NewList* nl, int32_t* __restrict__ Fn, uint32_t* __restrict__ eoffn,
                                          unsigned long long* out_counter) {
  __shared__ unsigned long long s_scan[4];
  __shared__ unsigned long long s_base;
  __syncthreads();
  const uint32_t cnt = nl->count;
  if (cnt == 0) return;  // uniform
  const int tid = threadIdx.x;
  // each thread owns up to 9 consecutive collected entries (2049 / 256 rounded up)
  constexpr int kPer = (kPushTile + 1 + 255) / 256;
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

// (the body of k_sparse_push for workgroup `bid` of `nblk`, see sparse_prepare_body)
template <int MODE>
__device__ __forceinline__ void sparse_push_body(const int32_t* __restrict__ F, const double* __restrict__ cF,
                                                 const uint32_t* __restrict__ eoff, const uint32_t* __restrict__ trp,
                                                 const int32_t* __restrict__ tci,
                                                 const unsigned long long* __restrict__ out_ext,
                                                 const uint32_t* __restrict__ in_rp, double* __restrict__ res,
                                                 uint8_t* __restrict__ flags, uint32_t* __restrict__ armed,
                                                 int32_t* __restrict__ Fn, uint32_t* __restrict__ eoffn, DevCounters* ctr,
                                                 int level, int dead_slot, unsigned long long comb_min,
                                                 unsigned long long pk, const PushArgs& a, uint32_t bid, uint32_t nblk) {
  __shared__ uint32_t s_eoff[kStageCap + 1];
  __shared__ uint32_t s_row[kStageCap];
  __shared__ double s_c[kStageCap];
  __shared__ uint32_t s_i0;
  __shared__ NewList s_new;
  __shared__ int32_t s_key[kCombSlots];
  __shared__ double s_val[kCombSlots];
  const int tid = threadIdx.x;
  const uint32_t nf = (uint32_t)(pk >> kPackShift);
  const unsigned long long E = pk & kPackMask;
  unsigned long long* out_counter = &ctr->hist[level + 1];
  // Levels with enough edges to repeat destinations (hubs collect a large share of any R-MAT frontier's edges) sum
  // a tile's contributions per destination in LDS first, so a destination costs one returning global atomic and one
  // degree gather per tile instead of one per edge; small levels go straight to memory.
  const bool combine = E >= comb_min;
  if (tid == 0) s_new.count = 0;
  if (combine)
    for (int j = tid; j < kCombSlots; j += 256) {
      s_key[j] = -1;
      s_val[j] = 0.0;
    }
  __syncthreads();

  if (MODE != kBackward && bid == 0 && a.src >= 0) {
    // dead-end mass of this level lands on the source (Forward_Push.java:101-113; seed sets: k_seed_land_sparse)
    if (tid == 0) {
      const double dead = ctr->dead[dead_slot];
      if (dead > 0.0) {
        push_one<MODE>(a.src, dead, out_ext, in_rp, res, flags, armed, &s_new, a);
        ctr->dead[dead_slot] = 0.0;
      }
    }
    flush_new(&s_new, Fn, eoffn, out_counter);
  }

  const unsigned long long n_tiles = (E + kPushTile - 1) / kPushTile;
  for (unsigned long long t = bid; t < n_tiles; t += nblk) {
    const unsigned long long tile_lo = t * kPushTile;
    const unsigned long long tile_hi = (tile_lo + kPushTile < E) ? tile_lo + kPushTile : E;
    if (tid == 0) {  // last frontier index whose edge range starts at or before tile_lo
      uint32_t lo = 0, hi = nf;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((unsigned long long)eoff[mid] <= tile_lo) lo = mid + 1; else hi = mid;
      }
      s_i0 = lo - 1;
    }
    __syncthreads();
    uint32_t ci0 = s_i0;
    unsigned long long ce = tile_lo;
    while (ce < tile_hi) {
      const uint32_t cnt = (nf - ci0 < (uint32_t)kStageCap) ? nf - ci0 : (uint32_t)kStageCap;
      if (cnt == 0) break;
      for (uint32_t j = tid; j <= cnt; j += 256) {
        const uint32_t idx = ci0 + j;
        s_eoff[j] = idx < nf ? eoff[idx] : (uint32_t)E;
        if (j < cnt) {
          s_row[j] = trp[F[idx]];
          s_c[j] = cF[idx];
        }
      }
      __syncthreads();
      const unsigned long long cov_hi = ((unsigned long long)s_eoff[cnt] < tile_hi) ? s_eoff[cnt] : tile_hi;
      // four edges per thread in flight: col_idx loads, then degree gathers, then atomics, then tests
      for (unsigned long long base = ce + tid; base < cov_hi; base += 1024) {
        int32_t u[4];
        double add[4], old[4];
        uint32_t du[4];
        bool valid[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned long long e = base + 256ull * q;
          valid[q] = e < cov_hi;
          u[q] = 0;
          add[q] = 0.0;
          if (valid[q]) {
            const uint32_t e32 = (uint32_t)e;
            uint32_t lo = 0, hi = cnt;  // last staged entry whose range starts at or before e
            while (lo < hi) {
              const uint32_t mid = (lo + hi) >> 1;
              if (s_eoff[mid] <= e32) lo = mid + 1; else hi = mid;
            }
            const uint32_t j = lo - 1;
            u[q] = tci[s_row[j] + (e32 - s_eoff[j])];
            add[q] = s_c[j];
          }
        }
        if (MODE == kBackward || !combine) {
#pragma unroll
          for (int q = 0; q < 4; ++q) du[q] = valid[q] ? (uint32_t)(out_ext[u[q]] >> 32) : 1u;
        }
        if (MODE == kBackward) {  // every edge's quotient rounds on its own (Backward_Search.java:84-85)
#pragma unroll
          for (int q = 0; q < 4; ++q) add[q] = add[q] / (double)du[q];
        }
        if (combine) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (valid[q] && comb_insert(s_key, s_val, u[q], add[q])) valid[q] = false;  // lands with its slot
          if (MODE != kBackward) {
#pragma unroll
            for (int q = 0; q < 4; ++q) du[q] = valid[q] ? (uint32_t)(out_ext[u[q]] >> 32) : 1u;  // table full
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          old[q] = 0.0;
          if (valid[q]) old[q] = atomic_add_ret(&res[u[q]], add[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (valid[q]) push_finish<MODE>(u[q], add[q], old[q], du[q], in_rp, flags, armed, &s_new, a);
      }
      __syncthreads();
      ce = cov_hi;
      ci0 += cnt;
    }
    if (combine) {
      // the tile's per-destination sums land: four slots per thread in flight, slots left empty for the next tile
      for (int j0 = tid; j0 < kCombSlots; j0 += 1024) {
        int32_t u[4];
        double add[4], old[4];
        uint32_t du[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          u[q] = s_key[j0 + 256 * q];
          add[q] = s_val[j0 + 256 * q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) du[q] = u[q] >= 0 ? (uint32_t)(out_ext[u[q]] >> 32) : 1u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          old[q] = 0.0;
          if (u[q] >= 0) {
            old[q] = atomic_add_ret(&res[u[q]], add[q]);
            s_key[j0 + 256 * q] = -1;
            s_val[j0 + 256 * q] = 0.0;
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (u[q] >= 0) push_finish<MODE>(u[q], add[q], old[q], du[q], in_rp, flags, armed, &s_new, a);
      }
    }
    flush_new(&s_new, Fn, eoffn, out_counter);
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_sparse_push(const int32_t* __restrict__ F, const double* __restrict__ cF,
                                                      const uint32_t* __restrict__ eoff,
                                                      const uint32_t* __restrict__ trp, const int32_t* __restrict__ tci,
                                                      const unsigned long long* __restrict__ out_ext,
                                                      const uint32_t* __restrict__ in_rp, double* __restrict__ res,
                                                      uint8_t* __restrict__ flags, uint32_t* __restrict__ armed,
                                                      int32_t* __restrict__ Fn,
                                                      uint32_t* __restrict__ eoffn, DevCounters* ctr, int level,
                                                      unsigned long long dense_thresh, int dead_slot,
                                                      unsigned long long comb_min, unsigned long long pk0, PushArgs a) {
  const unsigned long long pk = (level == 0 && pk0 != ~0ull) ? pk0 : ctr->hist[level];
  if (!level_runs(pk, level, dense_thresh)) return;
  sparse_push_body<MODE>(F, cF, eoff, trp, tci, out_ext, in_rp, res, flags, armed, Fn, eoffn, ctr, level, dead_slot, comb_min,
                         pk, a, blockIdx.x, gridDim.x);
}

// Several SMALL sparse levels in one launch, on one workgroup: levels first .. last of a batch, each as long as the
// level before it left a frontier that is worth a sparse level (level_runs) and small enough for one workgroup
// (entries + edges < wg_cap; the first level is the host's choice).  A top-k round's push is 8.4 levels on R-MAT 22, three
// quarters of them below 4 096 entries + edges (60 % below 512), and each cost two launches and ~21 us of stream time
// whatever its size; here a level costs its dependent memory accesses.  Between the levels (and between a level's two
// steps) the workgroup's waves meet at a barrier with a release fence before it and an acquire fence behind it: what one
// wave wrote - list entries, contributions, counters - the others read from L2.  The host reads the batch's counters
// as before and applies the same two rules to tell which levels ran.
template <int MODE>
__global__ __launch_bounds__(256) void k_sparse_levels_wg(int32_t* F0, int32_t* F1, uint32_t* eoff0, uint32_t* eoff1,
                                                           const uint32_t* __restrict__ out_rp, double* res,
                                                           double* reserve, double* cF, const uint32_t* __restrict__ trp,
                                                           const int32_t* __restrict__ tci,
                                                           const unsigned long long* __restrict__ out_ext,
                                                           const uint32_t* __restrict__ in_rp, uint8_t* flags,
                                                           uint32_t* armed, DevCounters* ctr, int fb0, int first, int last,
                                                           unsigned long long dense_thresh, unsigned long long wg_cap,
                                                           int dead_slot, unsigned long long comb_min,
                                                           unsigned long long pk0, PushArgs a) {
  for (int level = first; level <= last; ++level) {
    const unsigned long long pk =
        (level == 0 && pk0 != ~0ull)
            ? pk0
            : __hip_atomic_load(&ctr->hist[level], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!level_runs(pk, level, dense_thresh)) return;
    if (level > 0 && (pk >> kPackShift) + (pk & kPackMask) >= wg_cap) return;  // too large for one workgroup
    const int fb = fb0 ^ (level & 1);
    int32_t* const F = fb ? F1 : F0;
    int32_t* const Fn = fb ? F0 : F1;
    uint32_t* const eo = fb ? eoff1 : eoff0;
    uint32_t* const eon = fb ? eoff0 : eoff1;
    sparse_prepare_body<MODE>(F, out_rp, res, reserve, cF, CView{nullptr, 1, 0}, ctr, level, dead_slot, pk0, pk, a, 0u, 1u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    sparse_push_body<MODE>(F, cF, eo, trp, tci, out_ext, in_rp, res, flags, armed, Fn, eon, ctr, level, dead_slot, comb_min, pk,
                           a, 0u, 1u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
}

// A sparse level's dead-end mass x lands on p, between the level's prepare and push kernels (the push kernel's inline
// landing on a.src stays off: a.src = -1): r(i) += x q_i with push_one's threshold test, enqueue and parking for every
// live seed, reserve(j) += x e_j for every dead-end seed.  Runs iff the level runs (level_runs), returns at once when the
// level returned no mass.
template <int MODE>
__global__ __launch_bounds__(256) void k_seed_land_sparse(const int32_t* __restrict__ id, const double* __restrict__ w,
                                                           uint32_t n_live, uint32_t n_all, unsigned int* done,
                                                           const unsigned long long* __restrict__ out_ext,
                                                           const uint32_t* __restrict__ in_rp, double* __restrict__ res,
                                                           double* __restrict__ reserve, uint8_t* __restrict__ flags,
                                                           uint32_t* __restrict__ armed, int32_t* __restrict__ Fn,
                                                           uint32_t* __restrict__ eoffn, DevCounters* ctr, int level,
                                                           unsigned long long dense_thresh, int dead_slot,
                                                           unsigned long long pk0, PushArgs a) {
  __shared__ NewList s_new;
  const unsigned long long pk = (level == 0 && pk0 != ~0ull) ? pk0 : ctr->hist[level];
  if (!level_runs(pk, level, dense_thresh)) return;
  const double x = ctr->dead[dead_slot];
  if (!(x > 0.0)) return;
  if (threadIdx.x == 0) s_new.count = 0;
  __syncthreads();
  for (uint32_t base = blockIdx.x * blockDim.x; base < n_all; base += gridDim.x * blockDim.x) {  // (uniform trip count)
    const uint32_t i = base + threadIdx.x;
    if (i < n_live)
      push_one<MODE>(id[i], x * w[i], out_ext, in_rp, res, flags, armed, &s_new, a);
    else if (i < n_all)
      reserve[id[i]] = reserve[id[i]] + x * w[i];  // (a dead-end seed is listed once; nothing else writes reserve now)
    flush_new(&s_new, Fn, eoffn, &ctr->hist[level + 1]);
  }
  seed_land_done(done, ctr, dead_slot);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// edges from which a level sums its tiles in the LDS table (the override exists for the tests, which run the table on
// graphs far below the default switch-over)
static unsigned long long comb_min_edges() {
  const char* comb_env = hook_env("PPRHIP_COMB_MIN_EDGES");
  return comb_env ? strtoull(comb_env, nullptr, 10) : (unsigned long long)kCombMinEdges;
}

// the CSR a level pushes along: forward over the out-edges, backward over the in-edges
static std::pair<const uint32_t*, const int32_t*> push_csr(const GraphData* D, int mode) {
  if (mode == kBackward) return {D->in_rp, D->in_ci};
  return {D->out_rp, D->out_ci};
}

int launch_sparse_prepare(pprhip_graph* g, const PushArgs& a, int fbuf, int level, uint64_t nf_upper,
                          unsigned long long dense_thresh, bool scatter_dense, int cbuf, int dead_slot,
                          unsigned long long pk0) {
  const uint32_t grid = grid_for(nf_upper, 256, 512);
  const CView cd = scatter_dense ? cview(g, cbuf) : CView{nullptr, 1, 0};
  DISPATCH_MODE(a.mode, k_sparse_prepare<M><<<dim3(grid), dim3(256), 0, g->stream>>>(
                            g->F[fbuf], g->gr->out_rp, g->residue, g->reserve, g->cF, cd, g->ctr, level, dense_thresh,
                            dead_slot, pk0, a));
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_sparse_push(pprhip_graph* g, const PushArgs& a, int fbuf, int level, uint64_t ef_upper,
                       unsigned long long dense_thresh, int dead_slot, unsigned long long pk0) {
  const uint32_t grid = grid_for(ef_upper, kPushTile, 2048);
  const auto [trp, tci] = push_csr(g->gr, a.mode);
  DISPATCH_MODE(a.mode, k_sparse_push<M><<<dim3(grid), dim3(256), 0, g->stream>>>(
                            g->F[fbuf], g->cF, g->eoff[fbuf], trp, tci, g->gr->out_ext, g->gr->in_rp, g->residue, g->flags,
                            g->armed, g->F[fbuf ^ 1], g->eoff[fbuf ^ 1], g->ctr, level, dense_thresh, dead_slot,
                            comb_min_edges(), pk0, a));
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_sparse_levels_wg(pprhip_graph* g, const PushArgs& a, int fbuf0, int first, int last,
                            unsigned long long dense_thresh, unsigned long long wg_cap, int dead_slot,
                            unsigned long long pk0) {
  const auto [trp, tci] = push_csr(g->gr, a.mode);
  DISPATCH_MODE(a.mode, k_sparse_levels_wg<M><<<dim3(1), dim3(256), 0, g->stream>>>(
                            g->F[0], g->F[1], g->eoff[0], g->eoff[1], g->gr->out_rp, g->residue, g->reserve, g->cF, trp, tci,
                            g->gr->out_ext, g->gr->in_rp, g->flags, g->armed, g->ctr, fbuf0, first, last, dense_thresh,
                            wg_cap, dead_slot, comb_min_edges(), pk0, a));
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_seed_land_sparse(pprhip_graph* g, const PushArgs& a, int fbuf, int level, unsigned long long dense_thresh,
                            int dead_slot, unsigned long long pk0) {
  const SeedTable* sd = g->seeds;
  const uint32_t n_all = sd->n_live + sd->n_dead;
  const uint32_t grid = grid_for(n_all, 256, 1024);
  DISPATCH_MODE(a.mode, k_seed_land_sparse<M><<<dim3(grid), dim3(256), 0, g->stream>>>(
                            sd->id, sd->w, sd->n_live, n_all, sd->done, g->gr->out_ext, g->gr->in_rp, g->residue, g->reserve,
                            g->flags, g->armed, g->F[fbuf ^ 1], g->eoff[fbuf ^ 1], g->ctr, level, dense_thresh, dead_slot,
                            pk0, a));
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// Current device: this file's code object loaded.  Called once per device under the graph-lift lock (graph.cpp:
// init_device_once, which calls every file's init_kernels_*), never from a launch path.
int init_kernels_push() {
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_sparse_push<kBackward>)));
  return PPRHIP_OK;
}

}  // namespace pprhip
