// kernels_weighted_batch.hip — the dense level of sixteen WEIGHTED queries at once for gfx950 (MI355X): the batched
// sweep of kernels_dense_batch.hip over P(u, v) = w / W(u) (DESIGN.md §2 "Batched weighted FORA"; weighted_batch.cpp
// drives them).  The contributions of the kBatch queries in flight are interleaved, c8[v][slot] - one 128-byte line per
// vertex - in the batch state's arrays, the row sums in acc8[row ordinal][slot]; residue and reserve stay the slots' own
// vectors (SlotArgs).
//
//   k_wbat_edges    a wave owns a chunk of 512 in-edges as in k_w_dense_edges: in_ci and in_w are streamed once,
//                   non-temporally, 8 edges per lane.  The lanes work as in k_dense_edges_b: G = 16 lanes (one per slot)
//                   share an edge, lane group g walks edges [128 g, 128 (g + 1)) of the chunk; an edge's index and weight
//                   come out of the owning lane's registers with ds_swizzle, the gather brings the source's line, and
//                   the term is c[src][slot] * w(e) - the product k_w_dense_edges forms.  Only rows that cross the chunk
//                   boundary use atomics on acc8.  No LDS.
//   k_wbat_apply    k_w_dense_apply<false, *> per (row, slot): 64 rows at a time through an LDS tile [row][slot], so that
//                   acc8 and c8 move as whole lines while a wave walks a slot's residue / reserve with a lane per row.
//                   An idle column gets zeros.  k_wbat_apply_extra: the rows without in-edges a column still has to visit
//                   (its source, or its live seeds without in-edges), one workgroup per column.
//   k_wbat_reduce   the per-workgroup partials of every column into the slot's counters and into sweep_out.
//   k_wbat_scatter  k_w_prepare writing c with stride kBatch: a slot's frontier list enters its column.
//   k_wbat_compact  a column back to list form (and handed back all-zero): launch_compact_prepared for cdense.
//   k_wbat_leave    the column's entries on the rows k_wbat_apply does not rewrite, zeroed in both arrays.
//   k_wbat_collect  the counters a round of the driver waits for, side by side in sweep_out: one read-back per round.
//
// All arithmetic is IEEE double with -ffp-contract=off, c = ((1 - alpha) * r) / W(v), a term is c * w(e): batching
// changes the order of additions and nothing else (tests/weighted_ref.py).
#include "weighted_device.hpp"

namespace pprhip {

constexpr int kWbatG = kBatch;  // lanes per edge = slots
static_assert(kWbatG == 16, "the lane groups of k_wbat_edges and the flag words they read are laid out for sixteen slots");

// value of lane K of the caller's lane group of 16
template <int K>
__device__ __forceinline__ int wbat_bcast(int x) {
  return __builtin_amdgcn_ds_swizzle(x, (0x1f & ~(kWbatG - 1)) | (K << 5));
}
template <int K>
__device__ __forceinline__ double wbat_bcast_f64(double x) {
  return __hiloint2double(wbat_bcast<K>(__double2hiint(x)), wbat_bcast<K>(__double2loint(x)));
}

struct WbatChunkRegs {  // one lane's share of a chunk: 8 indices, their weights; the row-start bits of its group's 128 edges
  int4 ia, ib;
  double w[8];
  unsigned long long mask[2];
};

__device__ __forceinline__ WbatChunkRegs wbat_load_chunk(const int32_t* __restrict__ in_ci, const double* __restrict__ in_w,
                                                     const unsigned long long* __restrict__ flags64, uint32_t c, int lane) {
  const unsigned long long e0 = (unsigned long long)c * kChunkEdges + 8ull * lane;
  // both streams are read once per sweep: non-temporal, so that they do not push gathered lines out of L2
  typedef int v4i __attribute__((ext_vector_type(4)));
  typedef double v2d __attribute__((ext_vector_type(2)));
  const v4i* q = reinterpret_cast<const v4i*>(in_ci + e0);
  const v2d* qw = reinterpret_cast<const v2d*>(in_w + e0);
  const v4i x = __builtin_nontemporal_load(q), y = __builtin_nontemporal_load(q + 1);
  const v2d w0 = __builtin_nontemporal_load(qw), w1 = __builtin_nontemporal_load(qw + 1),
            w2 = __builtin_nontemporal_load(qw + 2), w3 = __builtin_nontemporal_load(qw + 3);
  WbatChunkRegs r;
  r.ia = make_int4(x.x, x.y, x.z, x.w);
  r.ib = make_int4(y.x, y.y, y.z, y.w);
  r.w[0] = w0.x; r.w[1] = w0.y; r.w[2] = w1.x; r.w[3] = w1.y;
  r.w[4] = w2.x; r.w[5] = w2.y; r.w[6] = w3.x; r.w[7] = w3.y;
  const size_t f0 = (size_t)c * 8 + (size_t)(lane / kWbatG) * 2;
  r.mask[0] = __builtin_nontemporal_load(&flags64[f0]);
  r.mask[1] = __builtin_nontemporal_load(&flags64[f0 + 1]);
  return r;
}

// 8 edges of the group: their indices and weights sit in lane JB of the group
template <int JB>
__device__ __forceinline__ void wbat_edges_block(const WbatChunkRegs& cur, const double* __restrict__ cB, int s, uint32_t before,
                                               double* __restrict__ accB, double& seg, double& first_seg, uint32_t& k) {
  const int32_t own[8] = {cur.ia.x, cur.ia.y, cur.ia.z, cur.ia.w, cur.ib.x, cur.ib.y, cur.ib.z, cur.ib.w};
  uint32_t v[8];
  double w[8], val[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (uint32_t)wbat_bcast<JB>(own[i]);
#pragma unroll
  for (int i = 0; i < 8; ++i) val[i] = cB[(size_t)v[i] * kWbatG + s];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = wbat_bcast_f64<JB>(cur.w[i]);
#pragma unroll
  for (int i = 0; i < 8; ++i) val[i] = val[i] * w[i];  // (a padding edge: source 0, weight 0.0)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if ((cur.mask[(JB * 8 + i) >> 6] >> ((JB * 8 + i) & 63)) & 1ull) {
      if (k == 0)
        first_seg = seg;  // closes the row carried in from earlier groups
      else
        __builtin_nontemporal_store(seg, &accB[(size_t)(before + k - 1) * kWbatG + s]);  // starts and ends inside this group
      seg = 0.0;
      ++k;
    }
    seg += val[i];
  }
}

template <int JB>
struct WbatEdgeBlocks {
  static __device__ __forceinline__ void run(const WbatChunkRegs& cur, const double* __restrict__ cB, int s, uint32_t before,
                                             double* __restrict__ accB, double& seg, double& first_seg, uint32_t& k) {
    WbatEdgeBlocks<JB - 1>::run(cur, cB, s, before, accB, seg, first_seg, k);
    wbat_edges_block<JB>(cur, cB, s, before, accB, seg, first_seg, k);
  }
};
template <>
struct WbatEdgeBlocks<-1> {
  static __device__ __forceinline__ void run(const WbatChunkRegs&, const double*, int, uint32_t, double*, double&, double&,
                                             uint32_t&) {}
};

// ------------------------------------------------------------------------------------------------
// the batched weighted sweep: edges
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_wbat_edges(const int32_t* __restrict__ in_ci, const double* __restrict__ in_w,
                                                   const unsigned long long* __restrict__ flags64,
                                                   const uint32_t* __restrict__ chunk_starts, uint32_t n_chunks,
                                                   const double* __restrict__ cB, double* __restrict__ accB) {
  const int lane = lane_id();
  const int grp = lane / kWbatG, s = lane & (kWbatG - 1);
  const uint32_t waves_per_block = blockDim.x >> 6;
  const uint32_t stride = gridDim.x * waves_per_block;
  uint32_t c = blockIdx.x * waves_per_block + (uint32_t)__builtin_amdgcn_readfirstlane(wave_id());
  if (c >= n_chunks) return;
  WbatChunkRegs cur = wbat_load_chunk(in_ci, in_w, flags64, c, lane);
  for (; c < n_chunks; c += stride) {
    // the next chunk's streams are requested before this chunk's gathers, so their latency is hidden
    WbatChunkRegs nxt = cur;
    if (c + stride < n_chunks) nxt = wbat_load_chunk(in_ci, in_w, flags64, c + stride, lane);
    const uint32_t cs = chunk_starts[c];
    const uint32_t pc = (uint32_t)__popcll(cur.mask[0]) + (uint32_t)__popcll(cur.mask[1]);
    const uint32_t incl = wave_incl_scan_u32_dpp(s == 0 ? pc : 0u);  // row starts up to and including this group
    const uint32_t before = cs + incl - pc;
    double seg = 0.0, first_seg = 0.0;
    uint32_t k = 0;
    WbatEdgeBlocks<kWbatG - 1>::run(cur, cB, s, before, accB, seg, first_seg, k);
    // segmented scan over the lane groups: S(g) = tail(g) + (group g holds a row start ? 0 : S(g-1))
    const bool h = k != 0;
    double S = seg;
    int F = h ? 1 : 0;
#pragma unroll
    for (int d = kWbatG; d < 64; d <<= 1) {
      const double ps = __shfl_up(S, d);
      const int pf = __shfl_up(F, d);
      if (lane >= d) {
        if (!F) S += ps;
        F |= pf;
      }
    }
    double carry = __shfl_up(S, kWbatG);
    if (lane < kWbatG) carry = 0.0;
    const unsigned long long hmask = __ballot(h);
    if (h) {
      // the row that ends at this group's first start flag: edges carried in + this group's head
      const bool nonempty = grp > 0 || (cur.mask[0] & 1ull) == 0;
      if (nonempty && before > 0) {
        const double total = carry + first_seg;
        const bool started_here = (hmask & ((1ull << (grp * kWbatG)) - 1ull)) != 0;  // an earlier group starts a row
        double* dst = &accB[(size_t)(before - 1) * kWbatG + s];
        if (started_here)
          *dst = total;
        else
          atomic_add_noret(dst, total);  // began in an earlier chunk
      }
    }
    if (grp == 64 / kWbatG - 1) {  // the row still open at the end of the chunk
      const uint32_t starts = cs + incl;
      if (starts > 0 && S != 0.0) atomic_add_noret(&accB[(size_t)(starts - 1) * kWbatG + s], S);
    }
    cur = nxt;
  }
}

// ------------------------------------------------------------------------------------------------
// the batched weighted sweep: apply
// ------------------------------------------------------------------------------------------------
constexpr int kWbatRows = 64;       // rows of a tile
constexpr int kWbatThreads = 256;   // 4 waves, 4 slots each
constexpr int kWbatSlotsPerWave = kBatch / (kWbatThreads / 64);
constexpr int kWbatPerThread = kWbatRows * kBatch / kWbatThreads;

struct WbatRowOut {  // what a wave's rows leave for one slot
  double dead_next = 0.0;
  unsigned long long pack = 0, ndead = 0;
};

// k_w_dense_apply<false, *>'s row: the row sum `acc` of row u lands (with the slot's returned dead-end mass: on its
// source, or - a seed set - as x * seed_w[u], the cell left for the landing kernel behind), the threshold is tested with
// the relationship count, a crossing row is prepared in place.  Returns c_next[u][slot].
__device__ __forceinline__ double wbat_apply_row(const SlotArgs& a, int32_t u, double acc,
                                               const unsigned long long* __restrict__ out_ext,
                                               const double* __restrict__ wsum, WbatRowOut& o) {
  if (a.seed_w) {
    const double q = a.seed_w[u];
    if (q != 0.0) {
      const double dd = a.ctr->dead[a.dead_slot];
      if (dd > 0.0) acc += dd * q;
    }
  } else if (u == a.src) {
    const double dd = a.ctr->dead[a.dead_slot];
    if (dd > 0.0) {
      acc += dd;
      a.ctr->dead[a.dead_slot] = 0.0;
    }
  }
  double cn = 0.0;
  if (acc > 0.0) {
    const uint32_t d = (uint32_t)(out_ext[u] >> 32);
    const double old = a.res[u];
    const double nw = old + acc;
    const bool crossing = !active_fwd(old, d, a.rmax) && active_fwd(nw, d, a.rmax);
    if (crossing) {  // becomes a frontier node of the next level: prepare it right here
      a.reserve[u] = a.reserve[u] + nw * a.alpha;
      if (old != 0.0) a.res[u] = 0.0;
      if (d == 0) {
        o.dead_next += nw * (1.0 - a.alpha);
        o.ndead++;
      } else {
        cn = ((1.0 - a.alpha) * nw) / wsum[u];
      }
      o.pack += (1ull << kPackShift) | (unsigned long long)d;
    } else {
      a.res[u] = nw;
    }
  }
  return cn;
}

__global__ __launch_bounds__(kWbatThreads) void k_wbat_apply(const int32_t* __restrict__ nz_rows, uint32_t n_nz,
                                                          double* __restrict__ acc8,
                                                          const unsigned long long* __restrict__ out_ext,
                                                          const double* __restrict__ wsum, double* __restrict__ c8_next,
                                                          const SlotArgs* __restrict__ slots,
                                                          unsigned long long* __restrict__ blk_pack8,
                                                          double* __restrict__ blk_dead8, uint32_t* __restrict__ blk_ndead8,
                                                          uint32_t part_stride) {
  __shared__ double tile[kWbatRows][kBatch + 1];
  __shared__ int32_t s_u[kWbatRows];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the slot arguments load into SGPRs
  SlotArgs a[kWbatSlotsPerWave];
  WbatRowOut o[kWbatSlotsPerWave];
#pragma unroll
  for (int i = 0; i < kWbatSlotsPerWave; ++i) a[i] = slots[w * kWbatSlotsPerWave + i];
  const uint32_t n_tiles = (n_nz + kWbatRows - 1) / kWbatRows;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t j0 = t * kWbatRows;
    // the tile's row sums come in as whole lines; every entry met non-zero is cleared (the rows that cross a chunk
    // boundary are summed with atomics, the others are rewritten by plain stores every sweep)
#pragma unroll
    for (int i = 0; i < kWbatPerThread; ++i) {
      const uint32_t idx = (uint32_t)i * (uint32_t)kWbatThreads + tid;
      const uint32_t r = idx / kBatch, s = idx % kBatch, j = j0 + r;
      double v = 0.0;
      if (j < n_nz) {
        v = acc8[(size_t)j * kBatch + s];
        if (v != 0.0) acc8[(size_t)j * kBatch + s] = 0.0;
      }
      tile[r][s] = v;
    }
    if (tid < kWbatRows) s_u[tid] = j0 + tid < n_nz ? nz_rows[j0 + tid] : -1;
    __syncthreads();
    const int32_t u = s_u[lane];
#pragma unroll
    for (int i = 0; i < kWbatSlotsPerWave; ++i) {
      const int s = w * kWbatSlotsPerWave + i;
      double cn = 0.0;
      if (a[i].active && u >= 0) cn = wbat_apply_row(a[i], u, tile[lane][s], out_ext, wsum, o[i]);
      tile[lane][s] = cn;  // (an idle column: zeros)
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kWbatPerThread; ++i) {
      const uint32_t idx = (uint32_t)i * (uint32_t)kWbatThreads + tid;
      const uint32_t r = idx / kBatch, s = idx % kBatch;
      const int32_t ur = s_u[r];
      if (ur >= 0) c8_next[(size_t)ur * kBatch + s] = tile[r][s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < kWbatSlotsPerWave; ++i) {
    const double ds = wave_sum_f64(o[i].dead_next);
    const unsigned long long ps = wave_sum_u64(o[i].pack);
    const unsigned long long nd = wave_sum_u64(o[i].ndead);
    // per-workgroup partials, one per wave's slot: k_wbat_reduce sums them (no same-address atomics in this kernel)
    if (lane == 0) {
      const size_t p = (size_t)(w * kWbatSlotsPerWave + i) * part_stride + blockIdx.x;
      blk_pack8[p] = ps;
      blk_dead8[p] = ds;
      blk_ndead8[p] = (uint32_t)nd;
    }
  }
}

// The rows without in-edges a column visits (launch_w_dense_level's extra rows): its source when that has no in-edges -
// it only ever receives returned dead-end mass - or, a seed set, its live seeds without in-edges.  Workgroup = column;
// its partial goes behind k_wbat_apply's (index part_at).
struct WbatExtra {
  const int32_t* list[kBatch];  // a seed set's rows; nullptr: `single`
  int32_t single[kBatch];       // the source without in-edges, or -1
  uint32_t n[kBatch];
};

__global__ __launch_bounds__(256) void k_wbat_apply_extra(WbatExtra x, const unsigned long long* __restrict__ out_ext,
                                                         const double* __restrict__ wsum, double* __restrict__ c8_next,
                                                         const SlotArgs* __restrict__ slots,
                                                         unsigned long long* __restrict__ blk_pack8,
                                                         double* __restrict__ blk_dead8, uint32_t* __restrict__ blk_ndead8,
                                                         uint32_t part_stride, uint32_t part_at) {
  __shared__ double s_red[4];
  __shared__ unsigned long long s_red2[4];
  const int s = blockIdx.x;
  const SlotArgs a = slots[s];
  WbatRowOut o;
  if (a.active) {
    const uint32_t cnt = x.list[s] ? x.n[s] : (x.single[s] >= 0 ? 1u : 0u);
    for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
      const int32_t u = x.list[s] ? x.list[s][i] : x.single[s];
      c8_next[(size_t)u * kBatch + s] = wbat_apply_row(a, u, 0.0, out_ext, wsum, o);
    }
  }
  const double ds = block_sum_f64(o.dead_next, s_red);
  const unsigned long long ps = block_sum_u64(o.pack, s_red2);
  const unsigned long long nd = block_sum_u64(o.ndead, s_red2);
  if (threadIdx.x == 0) {
    const size_t p = (size_t)s * part_stride + part_at;
    blk_pack8[p] = ps;
    blk_dead8[p] = ds;
    blk_ndead8[p] = (uint32_t)nd;
  }
}

// workgroup s sums column s's partials into that slot's counters (k_dense_reduce_batch)
__global__ __launch_bounds__(1024) void k_wbat_reduce(const unsigned long long* __restrict__ blk_pack8,
                                                    const double* __restrict__ blk_dead8,
                                                    const uint32_t* __restrict__ blk_ndead8, uint32_t n_blocks,
                                                    uint32_t part_stride, const SlotArgs* __restrict__ slots,
                                                    unsigned long long* __restrict__ sweep_out) {
  __shared__ double s_red[16];
  __shared__ unsigned long long s_red2[16];
  const SlotArgs a = slots[blockIdx.x];
  if (!a.active) return;
  unsigned long long pack = 0, ndead = 0;
  double dead = 0.0;
  for (uint32_t i = threadIdx.x; i < n_blocks; i += blockDim.x) {
    pack += blk_pack8[(size_t)blockIdx.x * part_stride + i];
    dead += blk_dead8[(size_t)blockIdx.x * part_stride + i];
    ndead += blk_ndead8[(size_t)blockIdx.x * part_stride + i];
  }
  const unsigned long long ps = block_sum_u64(pack, s_red2);
  const unsigned long long nd = block_sum_u64(ndead, s_red2);
  const double ds = block_sum_f64(dead, s_red);
  if (threadIdx.x == 0) {
    a.ctr->packed[a.out_slot] = ps;
    sweep_out[blockIdx.x] = ps;
    if (nd) {
      a.ctr->dead[a.dead_slot ^ 1] = a.ctr->dead[a.dead_slot ^ 1] + ds;
      a.ctr->dead_pops += nd;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// entering and leaving a column
// ------------------------------------------------------------------------------------------------
// k_w_prepare with the contributions written into column `col` of the interleaved array (all-zero beforehand)
__global__ __launch_bounds__(256) void k_wbat_scatter(const int32_t* __restrict__ F, uint32_t nf,
                                                     const unsigned long long* __restrict__ out_ext,
                                                     const double* __restrict__ wsum, double* __restrict__ res,
                                                     double* __restrict__ reserve, double* __restrict__ c8, uint32_t col,
                                                     DevCounters* ctr, int dead_slot, double alpha) {
  __shared__ double s_red[4];
  __shared__ unsigned long long s_red2[4];
  double dead = 0.0;
  unsigned long long ndead = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
    const int32_t v = F[i];
    const double rc = res[v];
    res[v] = 0.0;
    reserve[v] = reserve[v] + rc * alpha;
    const uint32_t d = (uint32_t)(out_ext[v] >> 32);
    if (d == 0) {  // a dead end: the mass goes back to the source
      dead += rc * (1.0 - alpha);
      ndead++;
    } else {
      c8[(size_t)v * kBatch + col] = ((1.0 - alpha) * rc) / wsum[v];
    }
  }
  const double ds = block_sum_f64(dead, s_red);
  const unsigned long long nd = block_sum_u64(ndead, s_red2);
  if (threadIdx.x == 0 && nd) {
    atomic_add_noret(&ctr->dead[dead_slot], ds);
    atomic_add_u64(&ctr->dead_pops, nd);
  }
}

// column -> list: every node of [0, n) that holds a contribution, with the prefix of the out-degrees (k_w_push locates
// an edge by it) and its contribution; the column is handed back all-zero.  *counter: 0 before, entries << 36 | edges after.
__global__ __launch_bounds__(256) void k_wbat_compact(uint32_t n, double* __restrict__ c8, uint32_t col,
                                                     const unsigned long long* __restrict__ out_ext,
                                                     int32_t* __restrict__ Fn, uint32_t* __restrict__ eoffn,
                                                     double* __restrict__ cF, unsigned long long* counter) {
  const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
  const uint32_t lo = blockIdx.x * per;
  const uint32_t hi = lo + per < n ? lo + per : n;
  if (lo >= hi) return;
  block_range_compact(
      lo, hi, counter,
      [&](uint32_t v, unsigned long long* w) {
        if (!(c8[(size_t)v * kBatch + col] > 0.0)) return false;
        *w = out_ext[v] >> 32;
        return true;
      },
      [&](uint32_t v, uint32_t pos, unsigned long long eo, unsigned long long) {
        Fn[pos] = (int32_t)v;
        eoffn[pos] = (uint32_t)eo;
        cF[pos] = c8[(size_t)v * kBatch + col];
        c8[(size_t)v * kBatch + col] = 0.0;
      });
}

// The rows of a column that k_wbat_apply does not rewrite (k_wbat_apply_extra's rows) in both arrays: the array a sweep reads
// may hold what the sweep before left there.
__global__ __launch_bounds__(256) void k_wbat_leave(const int32_t* __restrict__ list, int32_t single, uint32_t cnt,
                                                   double* __restrict__ c8a, double* __restrict__ c8b, uint32_t col) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
    const int32_t u = list ? list[i] : single;
    c8a[(size_t)u * kBatch + col] = 0.0;
    c8b[(size_t)u * kBatch + col] = 0.0;
  }
}

struct WbatCells {
  const unsigned long long* cell[kBatch];  // nullptr: sweep_out[s] stays (the sweep's reduce wrote it, or nobody waits)
};
__global__ void k_wbat_collect(WbatCells c, unsigned long long* __restrict__ sweep_out) {
  const int s = threadIdx.x;
  if (s < kBatch && c.cell[s]) sweep_out[s] = *c.cell[s];
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// the rows of slot S's query that lie outside the sweep's rows: a seed set's live seeds without in-edges, or the source
// without in-edges
static void wbat_extra_of(const pprhip_graph* S, int32_t src, const int32_t** list, int32_t* single, uint32_t* n) {
  const GraphData* D = S->gr;
  *list = nullptr;
  *single = -1;
  *n = 0;
  if (src < 0) {  // a seed set (PushArgs::src is -1)
    const SeedTable* sd = S->seeds;
    if (sd && sd->n_zin) {
      *list = sd->zin;
      *n = sd->n_zin;
    }
  } else if (D->h_in_rp[src + 1] == D->h_in_rp[src]) {
    *single = src;
    *n = 1;
  }
}

int launch_wbat_scatter(pprhip_graph* S, const PushArgs& a, int fbuf, uint32_t nf, int dead_slot) {
  const BatchState* bs = S->parent->batch;
  k_wbat_scatter<<<dim3(grid_for(nf, 256, 512)), dim3(256), 0, S->stream>>>(
      S->F[fbuf], nf, S->gr->out_ext, S->gr->wsum, S->residue, S->reserve, bs->c8[bs->c8cur], (uint32_t)S->slot_index,
      S->ctr, dead_slot, a.alpha);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_wbat_compact(pprhip_graph* S, int out_fbuf, unsigned long long* d_counter) {
  const BatchState* bs = S->parent->batch;
  k_wbat_compact<<<dim3(grid_for(act_n(S), 1024, 1024)), dim3(256), 0, S->stream>>>(
      act_n(S), bs->c8[bs->c8cur], (uint32_t)S->slot_index, S->gr->out_ext, S->F[out_fbuf], S->eoff[out_fbuf], S->cF,
      d_counter);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_wbat_leave(pprhip_graph* S, int32_t src) {
  const BatchState* bs = S->parent->batch;
  const int32_t* list;
  int32_t single;
  uint32_t n;
  wbat_extra_of(S, src, &list, &single, &n);
  if (!n) return PPRHIP_OK;
  k_wbat_leave<<<dim3(grid_for(n, 256, 64)), dim3(256), 0, S->stream>>>(list, single, n, bs->c8[0], bs->c8[1],
                                                                     (uint32_t)S->slot_index);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// One batched weighted sweep of the columns marked active in the batch state's staged slot arguments (h_slot_args;
// SlotArgs::src as PushArgs::src): c8[c8cur] -> c8[c8cur ^ 1], every active column's new frontier counter into its
// slot's ctr->packed[out_slot] and into sweep_out, its next dead-end mass into ctr->dead[dead_slot ^ 1].
int launch_wbat_sweep(pprhip_graph* P) {
  const GraphData* D = P->gr;
  BatchState* bs = P->batch;
  PPRHIP_CHECK_HIP(hipMemcpyAsync(bs->d_slot_args, bs->h_slot_args, sizeof(SlotArgs) * kBatch, hipMemcpyHostToDevice,
                                  P->stream));
  if (D->n_chunks) {
    constexpr uint32_t kWaves = 8;  // per workgroup of 512 threads
    const uint32_t want = (D->n_chunks + kWaves - 1) / kWaves;
    const uint32_t grid = std::min<uint32_t>(want, (uint32_t)D->n_cus * 4u);
    k_wbat_edges<<<dim3(grid), dim3(64 * kWaves), 0, P->stream>>>(
        D->in_ci, D->in_w, reinterpret_cast<const unsigned long long*>(D->start_flags), D->chunk_starts, D->n_chunks,
        bs->c8[bs->c8cur], bs->acc8);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  const uint32_t n_tiles = (D->n_nz + kWbatRows - 1) / kWbatRows;
  const uint32_t grid = std::min<uint32_t>(n_tiles, kApplyBlocks8 - 1u);  // (one partial is the extra rows')
  if (grid) {
    k_wbat_apply<<<dim3(grid), dim3(kWbatThreads), 0, P->stream>>>(D->nz_rows, D->n_nz, bs->acc8, D->out_ext, D->wsum,
                                                              bs->c8[bs->c8cur ^ 1], bs->d_slot_args, bs->blk_pack8,
                                                              bs->blk_dead8, bs->blk_ndead8, kApplyBlocks8);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  WbatExtra x;
  for (int s = 0; s < kBatch; ++s) {
    x.list[s] = nullptr;
    x.single[s] = -1;
    x.n[s] = 0;
    if (bs->h_slot_args[s].active) wbat_extra_of(bs->slots[s], bs->h_slot_args[s].src, &x.list[s], &x.single[s], &x.n[s]);
  }
  k_wbat_apply_extra<<<dim3(kBatch), dim3(256), 0, P->stream>>>(x, D->out_ext, D->wsum, bs->c8[bs->c8cur ^ 1],
                                                              bs->d_slot_args, bs->blk_pack8, bs->blk_dead8,
                                                              bs->blk_ndead8, kApplyBlocks8, grid);
  PPRHIP_CHECK_HIP(hipGetLastError());
  // a seeded column: the dead-end seeds' share of the level's dead-end mass, and the cell cleared (the slots work on
  // the sweep's stream)
  for (int s = 0; s < kBatch; ++s)
    if (bs->h_slot_args[s].active && bs->h_slot_args[s].seed_w)
      PPRHIP_TRY(launch_wq_land_dense(bs->slots[s], bs->h_slot_args[s].dead_slot));
  k_wbat_reduce<<<dim3(kBatch), dim3(1024), 0, P->stream>>>(bs->blk_pack8, bs->blk_dead8, bs->blk_ndead8, grid + 1u,
                                                          kApplyBlocks8, bs->d_slot_args, bs->sweep_out);
  PPRHIP_CHECK_HIP(hipGetLastError());
  bs->c8cur ^= 1;
  return PPRHIP_OK;
}

int launch_wbat_collect(pprhip_graph* P, const unsigned long long* const* cells) {
  WbatCells c;
  for (int s = 0; s < kBatch; ++s) c.cell[s] = cells[s];
  k_wbat_collect<<<dim3(1), dim3(64), 0, P->stream>>>(c, P->batch->sweep_out);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int init_kernels_weighted_batch() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_wbat_edges)));
  return PPRHIP_OK;
}

}  // namespace pprhip
