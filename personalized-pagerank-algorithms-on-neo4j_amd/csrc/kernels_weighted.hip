// kernels_weighted.hip — weighted relationships for gfx950 (MI355X): the levels of a weighted forward push / power
// method and the weighted walks (DESIGN.md §2 "Weighted relationships"; weighted.cpp drives them).  The transition
// matrix is P(u, v) = sum of w(u -> v) / W(u); the weights are fp64 arrays beside the CSR pair (engine.hpp: GraphData).
// The unweighted kernels carry no weight branch: these are kernels of their own, modelled on them.
//
//   sparse  k_w_prepare (per frontier node: take the residue, credit the reserve, c = (1 - alpha) r / W) then k_w_push:
//           edge-parallel over the frontier's out-edges (frontier entries staged in LDS, an edge finds its entry by
//           binary search over the staged edge offsets, so a hub row is spread over lanes like any other), one
//           returning fp64 atomic per edge with add = c * w(e), threshold crossings on (old, old + add) collected in
//           LDS and appended to the next list with one packed atomic per tile.
//   dense   k_w_dense_edges: the flat pull sweep of kernels_dense.hip over in_ci / in_w - a wave owns 512 consecutive
//           in-edges, 8 per lane, index and weight streams read once (non-temporal), gathers c[src], multiplies, sums
//           by row with the segmented wave scan; row sums go to acc_nz.  k_w_dense_apply lands them (plus the dead-end
//           mass on the source), tests the threshold with the relationship COUNT and prepares crossing rows for the
//           next level; POWER: every row with mass pops; SEEDED: the mass lands on a seed table instead
//           (kernels_weighted_query.hip holds the rest of a seeded push).
//   walks   one walk per lane, refilled in ballot order; the neighbour pick is a binary search over the row's
//           inclusive weight prefix: x = (word * 2^-32) * W(cur), j = #{cum <= x} clamped to d - 1.
//   index   k_w_index_build stores the terminals of the walks a whole-graph weighted FORA phase draws per node (the
//           weighted walk index); a phase at the index's alpha and seed is served by kernels_walk.hip's k_index_serve
//           and k_w_walk_plan<true> walks only what the index does not hold.
//
// All arithmetic is IEEE double with -ffp-contract=off: each product / quotient rounds on its own, so that a host
// restatement of these rules (tests/weighted_ref.py) takes the same decisions.
#include <cstring>
#include <type_traits>

#include "weighted_device.hpp"

namespace pprhip {

// ------------------------------------------------------------------------------------------------
// sparse level, step 1: every frontier node gives up its residue
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_w_prepare(const int32_t* __restrict__ F, uint32_t nf,
                                                    const unsigned long long* __restrict__ out_ext,
                                                    const double* __restrict__ wsum, double* __restrict__ res,
                                                    double* __restrict__ reserve, double* __restrict__ cF,
                                                    double* __restrict__ c_dense, DevCounters* ctr, int dead_slot,
                                                    unsigned long long* next_counter, double alpha) {
  __shared__ double s_red[4];
  __shared__ unsigned long long s_red2[4];
  if (next_counter && blockIdx.x == 0 && threadIdx.x == 0) *next_counter = 0ull;  // the list k_w_push appends to
  double dead = 0.0;
  unsigned long long ndead = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
    const int32_t v = F[i];
    const double rc = res[v];
    res[v] = 0.0;
    reserve[v] = reserve[v] + rc * alpha;
    const uint32_t d = (uint32_t)(out_ext[v] >> 32);
    double c;
    if (d == 0) {  // a dead end: the mass goes back to the source, as in the unweighted push
      c = 0.0;
      dead += rc * (1.0 - alpha);
      ndead++;
    } else {
      c = ((1.0 - alpha) * rc) / wsum[v];  // every out-edge deposits c * w(e)
    }
    if (c_dense)
      c_dense[v] = c;
    else
      cF[i] = c;
  }
  const double ds = block_sum_f64(dead, s_red);
  const unsigned long long nd = block_sum_u64(ndead, s_red2);
  if (threadIdx.x == 0 && nd) {
    atomic_add_noret(&ctr->dead[dead_slot], ds);
    atomic_add_u64(&ctr->dead_pops, nd);
  }
}

// ------------------------------------------------------------------------------------------------
// sparse level, step 2: contributions land edge by edge
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_w_push(const int32_t* __restrict__ F, const double* __restrict__ cF,
                                                 const uint32_t* __restrict__ eoff, uint32_t nf, unsigned long long E,
                                                 const unsigned long long* __restrict__ out_ext,
                                                 const int32_t* __restrict__ out_ci, const double* __restrict__ out_w,
                                                 double* __restrict__ res, int32_t* __restrict__ Fn,
                                                 uint32_t* __restrict__ eoffn, DevCounters* ctr, int dead_slot,
                                                 unsigned long long* out_counter, int32_t src, double rmax) {
  __shared__ uint32_t s_eoff[kWStage + 1];
  __shared__ uint32_t s_row[kWStage];
  __shared__ double s_c[kWStage];
  __shared__ uint32_t s_i0;
  __shared__ WNewList s_new;
  const int tid = threadIdx.x;
  if (tid == 0) s_new.count = 0;
  __syncthreads();

  if (blockIdx.x == 0) {
    // dead-end mass of this level lands on the source, with the test a push applies
    if (tid == 0) {
      const double dead = ctr->dead[dead_slot];
      if (dead > 0.0) {
        const uint32_t ds = (uint32_t)(out_ext[src] >> 32);
        const double old = atomic_add_ret(&res[src], dead);
        w_push_finish(src, dead, old, ds, &s_new, rmax);
        ctr->dead[dead_slot] = 0.0;
      }
    }
    w_flush_new(&s_new, Fn, eoffn, out_counter);
  }

  const unsigned long long n_tiles = (E + kWTile - 1) / kWTile;
  for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const unsigned long long tile_lo = t * kWTile;
    const unsigned long long tile_hi = (tile_lo + kWTile < E) ? tile_lo + kWTile : E;
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
      const uint32_t cnt = (nf - ci0 < (uint32_t)kWStage) ? nf - ci0 : (uint32_t)kWStage;
      if (cnt == 0) break;
      for (uint32_t j = tid; j <= cnt; j += 256) {
        const uint32_t idx = ci0 + j;
        s_eoff[j] = idx < nf ? eoff[idx] : (uint32_t)E;
        if (j < cnt) {
          s_row[j] = (uint32_t)out_ext[F[idx]];  // first out-edge of the entry's row
          s_c[j] = cF[idx];
        }
      }
      __syncthreads();
      const unsigned long long cov_hi = ((unsigned long long)s_eoff[cnt] < tile_hi) ? s_eoff[cnt] : tile_hi;
      // four edges per thread in flight: col_idx and weight loads, then degree gathers, then atomics, then tests
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
            const uint32_t pos = s_row[j] + (e32 - s_eoff[j]);
            u[q] = out_ci[pos];
            add[q] = s_c[j] * out_w[pos];
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) du[q] = valid[q] ? (uint32_t)(out_ext[u[q]] >> 32) : 1u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          old[q] = 0.0;
          if (valid[q]) old[q] = atomic_add_ret(&res[u[q]], add[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (valid[q]) w_push_finish(u[q], add[q], old[q], du[q], &s_new, rmax);
      }
      __syncthreads();
      ce = cov_hi;
      ci0 += cnt;
    }
    w_flush_new(&s_new, Fn, eoffn, out_counter);
  }
}

// ------------------------------------------------------------------------------------------------
// dense level: flat pull sweep over in_ci / in_w
// ------------------------------------------------------------------------------------------------
// One wave per chunk of 512 consecutive in-edges (k_dense_edges<false, false> with the weight stream beside the index
// stream).  Padding edges carry source 0 and weight 0.0 and no row-start flag: they add 0 to the last row.  Rows that
// start and end inside the wave are stored, the (at most two) rows that cross the chunk boundary use an fp64 atomic on
// acc_nz, which k_w_dense_apply leaves zero.
__global__ __launch_bounds__(512) void k_w_dense_edges(const int32_t* __restrict__ in_ci, const double* __restrict__ in_w,
                                                        const uint8_t* __restrict__ start_flags,
                                                        const uint32_t* __restrict__ chunk_starts, uint32_t n_chunks,
                                                        const double* __restrict__ c_cur, double* __restrict__ acc_nz) {
  const int lane = lane_id();
  const uint32_t waves_per_block = blockDim.x >> 6;
  const uint32_t stride = gridDim.x * waves_per_block;
  uint32_t c = blockIdx.x * waves_per_block + (uint32_t)__builtin_amdgcn_readfirstlane(wave_id());
  if (c >= n_chunks) return;
  WChunkRegs cur = w_load_chunk(in_ci, in_w, start_flags, c, lane);
  for (; c < n_chunks; c += stride) {
    // the next chunk's streams are requested before this chunk's gathers, so their latency is hidden
    WChunkRegs nxt = cur;
    if (c + stride < n_chunks) nxt = w_load_chunk(in_ci, in_w, start_flags, c + stride, lane);
    const uint32_t cs = chunk_starts[c];
    const uint32_t fb = cur.fb;
    const int32_t idx[8] = {cur.ia.x, cur.ia.y, cur.ia.z, cur.ia.w, cur.ib.x, cur.ib.y, cur.ib.z, cur.ib.w};
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = c_cur[idx[i]];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = v[i] * cur.w[i];
    // row index of a segment = (row starts at or before its first edge) - 1
    const uint32_t pc = __popc(fb);
    const uint32_t incl = wave_incl_scan_u32_dpp(pc);
    const uint32_t before = cs + incl - pc;  // row starts before this lane's first edge
    double seg = 0.0, first_seg = 0.0;
    uint32_t k = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if ((fb >> i) & 1u) {
        if (k == 0)
          first_seg = seg;  // closes the row carried in from earlier lanes
        else
          acc_nz[before + k - 1] = seg;  // a row that starts and ends inside this lane
        seg = 0.0;
        ++k;
      }
      seg += v[i];
    }
    // segmented scan over lanes: S(l) = x(l) + (lane l holds a row start ? 0 : S(l-1))
    const bool h = k != 0;
    const double sval = wave_seg_scan_f64_dpp(seg, h);
    const double carry = wave_prev_f64_dpp(sval);
    const unsigned long long hmask = __ballot(h);
    if (h) {
      // the row that ends at this lane's first start flag: edges carried in + this lane's head
      const bool nonempty = lane > 0 || (fb & 1u) == 0;
      if (nonempty && before > 0) {
        const double tot = carry + first_seg;
        const bool started_here = (hmask & ((1ull << lane) - 1ull)) != 0;  // an earlier lane starts a row
        if (started_here)
          acc_nz[before - 1] = tot;
        else
          atomic_add_noret(&acc_nz[before - 1], tot);  // began in an earlier chunk
      }
    }
    if (lane == 63) {  // the row still open at the end of the chunk
      const uint32_t starts = cs + incl;
      if (starts > 0 && sval != 0.0) atomic_add_noret(&acc_nz[starts - 1], sval);
    }
    cur = nxt;
  }
}

// One thread per row with in-edges, plus one for a source without in-edges (it only ever receives returned dead-end
// mass): lands the row sum, tests the threshold and prepares a crossing row for the next level in place
// (k_dense_apply<kFwdWhole / kPower, false> with c = (1 - alpha) r / W).  POWER: every row with mass pops.
// SEEDED (a seed set, src = -1): the level's dead-end mass x lands on p - a row takes x * seed_w[u] (q of a live seed,
// zero elsewhere) before the test, the live seeds without in-edges are the extra rows, and the cell is left for
// k_wq_land_dense, which credits the dead-end seeds and clears it.
template <bool POWER, bool SEEDED>
__global__ __launch_bounds__(256) void k_w_dense_apply(const int32_t* __restrict__ nz_rows, uint32_t n_nz,
                                                        double* __restrict__ acc_nz,
                                                        const unsigned long long* __restrict__ out_ext,
                                                        const double* __restrict__ wsum, double* __restrict__ c_next,
                                                        double* __restrict__ res, double* __restrict__ reserve,
                                                        DevCounters* ctr, unsigned long long* __restrict__ blk_pack,
                                                        double* __restrict__ blk_dead, uint32_t* __restrict__ blk_ndead,
                                                        int dead_slot, int src_extra, int32_t src, double alpha,
                                                        double rmax, const double* __restrict__ seed_w,
                                                        const int32_t* __restrict__ extra_rows) {
  __shared__ double s_red[4];
  __shared__ unsigned long long s_red2[4];
  const int tid = threadIdx.x;
  const uint32_t j = blockIdx.x * 256u + tid;
  bool have = false;
  int32_t u = -1;
  double acc = 0.0;
  if (j < n_nz) {
    u = nz_rows[j];
    acc = acc_nz[j];
    acc_nz[j] = 0.0;
    have = true;
  } else if (j - n_nz < (uint32_t)src_extra) {
    u = SEEDED ? extra_rows[j - n_nz] : src;
    have = true;
  }
  double dead_next = 0.0;
  unsigned long long pack = 0, ndead = 0;
  if (have) {
    if (SEEDED) {
      const double q = seed_w[u];
      if (q != 0.0) {
        const double dd = ctr->dead[dead_slot];
        if (dd > 0.0) acc += dd * q;
      }
    } else if (u == src) {
      const double dd = ctr->dead[dead_slot];
      if (dd > 0.0) {
        acc += dd;
        ctr->dead[dead_slot] = 0.0;
      }
    }
    double cn = 0.0;
    if (acc > 0.0) {
      const uint32_t d = (uint32_t)(out_ext[u] >> 32);
      const double old = res[u];
      const double nw = old + acc;
      const bool crossing = POWER ? true : (!active_fwd(old, d, rmax) && active_fwd(nw, d, rmax));
      if (crossing) {  // becomes a frontier node of the next level: prepare it right here
        reserve[u] = reserve[u] + nw * alpha;
        if (old != 0.0) res[u] = 0.0;
        if (d == 0) {
          dead_next = nw * (1.0 - alpha);
          ndead = 1;
        } else {
          cn = ((1.0 - alpha) * nw) / wsum[u];
        }
        pack = (1ull << kPackShift) | (unsigned long long)d;
      } else {
        res[u] = nw;
      }
    }
    c_next[u] = cn;
  }
  // per-workgroup partials; k_dense_reduce sums them (no same-address atomics in this kernel)
  const double ds = block_sum_f64(dead_next, s_red);
  const unsigned long long ps = block_sum_u64(pack, s_red2);
  const unsigned long long nd = block_sum_u64(ndead, s_red2);
  if (tid == 0) {
    blk_pack[blockIdx.x] = ps;
    blk_dead[blockIdx.x] = ds;
    blk_ndead[blockIdx.x] = (uint32_t)nd;
  }
}

// pprhip_weighted_random_walk_batch: a wave owns a contiguous share of the call's walks; a lane whose walk has stopped
// writes its terminal and takes the wave's next walk (refill in ballot order, k_pair_walk's loop).
__global__ __launch_bounds__(256) void k_w_walk_batch(const int32_t* __restrict__ starts,
                                                       const unsigned long long* __restrict__ idx,
                                                       unsigned long long count, WWalkGraph G,
                                                       const int32_t* __restrict__ new2old, double alpha, uint32_t k0,
                                                       uint32_t k1, uint32_t stream, int no_zero_hop,
                                                       int32_t* __restrict__ term, uint32_t* __restrict__ steps) {
  const int lane = lane_id();
  const unsigned long long n_waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
  const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (unsigned long long)wave_id();
  const unsigned long long groups = (count + 63) / 64;
  const unsigned long long per = (groups + n_waves - 1) / n_waves * 64;
  unsigned long long cursor = wave * per;
  if (cursor >= count) return;
  const unsigned long long hi = cursor + per < count ? cursor + per : count;
  WWalker w;
  unsigned long long mine = 0;
  bool walking = false;
  for (;;) {
    const unsigned long long need = __ballot(!walking);
    if (need && cursor < hi) {
      const unsigned long long avail = hi - cursor;
      const uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
      if (!walking && rank < avail) {
        mine = cursor + rank;
        const int32_t s = starts[mine];
        const unsigned long long sext = G.out_ext[s];
        w_walker_init(w, s, sext, new2old[s], idx[mine], stream, no_zero_hop != 0);
        if ((sext >> 32) == 0) {  // a dead-end start is its own terminal
          term[mine] = s;
          if (steps) steps[mine] = 0u;
        } else {
          walking = true;
        }
      }
      const unsigned long long want = __popcll(need);
      cursor += want < avail ? want : avail;
    }
    if (__ballot(walking) == 0) {
      if (cursor >= hi) break;
      continue;
    }
    if (walking && w_walker_step(w, G, alpha, k0, k1)) {
      term[mine] = w.cur;
      if (steps) steps[mine] = w.moves;
      walking = false;
    }
  }
}

// The weighted walks of a plan (k_mc_plan<0> -> WalkPlanRec): one wave per workgroup with a contiguous share of the
// phase's walks, a lane takes the wave's next walk when its own has stopped (ballot order) and finds the walk's entry
// by binary search over the entries' walk offsets, from the entry of the wave's oldest open walk on.  The walks are
// (seed, stream, node, index within the entry), with or without the forced first hop (whole-graph FORA: stream 0,
// forced; a weighted top-k round: its round number, not forced); every walk adds its entry's increment at its terminal.
// INDEXED (idx_off: the offsets of the weighted walk index; k_mc_walk<kWalkIndexed>'s rule): k_index_serve has deposited
// the stored terminals of this plan and counted the walks the index does not hold into ctr->walks_over.  None: the
// kernel returns at once.  Otherwise a walk whose index lies below its node's capacity is passed over, the others - an
// entry's tail [cap, omega_i), every walk of a dead-end start - run with their own indices.  The plain instantiation is
// the kernel as it was, argument block included: its last argument is an empty struct, which takes no bytes there.
struct WNoIndex {};
template <bool INDEXED>
using WIndexOffsets = std::conditional_t<INDEXED, const unsigned long long*, WNoIndex>;

template <bool INDEXED>
__global__ __launch_bounds__(64) void k_w_walk_plan(const WalkPlanRec* __restrict__ plan_rec, WWalkGraph G,
                                                     double* __restrict__ target, double alpha, uint32_t k0, uint32_t k1,
                                                     uint32_t stream, int no_zero_hop, DevCounters* ctr, int parity,
                                                     WIndexOffsets<INDEXED> idx_off) {
  const unsigned long long plan = ctr->mc_plan[parity];
  const uint32_t n_src = (uint32_t)(plan >> kPackShift);
  const unsigned long long n_walks = plan & kPackMask;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctr->walks_total += n_walks;
    ctr->sources_total += n_src;
  }
  if (INDEXED && ctr->walks_over == 0ull) return;  // the index held every walk of the phase
  const int lane = threadIdx.x;
  const unsigned long long groups = (n_walks + 63) / 64;
  const unsigned long long per = (groups + gridDim.x - 1) / gridDim.x * 64;
  unsigned long long cursor = (unsigned long long)blockIdx.x * per;
  if (cursor >= n_walks || n_src == 0) return;
  const unsigned long long w_hi = cursor + per < n_walks ? cursor + per : n_walks;
  uint32_t e_lo = 0;  // an entry at or before the entry of walk `cursor` (wave-uniform)
  unsigned long long steps_total = 0;
  WWalker w;
  double inc = 0.0;
  bool walking = false;
  for (;;) {
    const unsigned long long need = __ballot(!walking);
    if (need && cursor < w_hi) {
      const unsigned long long avail = w_hi - cursor;
      const uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
      uint32_t e = e_lo;
      if (!walking && rank < avail) {
        const unsigned long long gidx = cursor + rank;
        // the last entry whose walk range starts at or before gidx (woff[0] = 0, woff[e_lo] <= cursor <= gidx)
        uint32_t a = e_lo + 1u, b = n_src;
        while (a < b) {
          const uint32_t mid = (a + b) >> 1;
          if (plan_rec[mid].woff <= gidx) a = mid + 1u; else b = mid;
        }
        e = a - 1u;
        const WalkPlanRec r = plan_rec[e];
        inc = r.inc;
        w_walker_init(w, r.node, r.ext, r.orig, gidx - r.woff, stream, no_zero_hop != 0);
        if ((r.ext >> 32) == 0)
          atomic_add_noret(&target[r.node], inc);  // a dead-end start is its own terminal
        else
          walking = true;
        if constexpr (INDEXED)  // k_index_serve has deposited this walk's terminal (never a dead-end start's: capacity 0)
          if (gidx - r.woff < idx_off[r.node + 1] - idx_off[r.node]) walking = false;
      }
      // the walk of the first refilled lane is the oldest one the wave has not placed yet
      e_lo = (uint32_t)__shfl((int)e, __builtin_ctzll(need));
      const unsigned long long want = __popcll(need);
      cursor += want < avail ? want : avail;
    }
    if (__ballot(walking) == 0) {
      if (cursor >= w_hi) break;
      continue;
    }
    if (walking && w_walker_step(w, G, alpha, k0, k1)) {
      atomic_add_noret(&target[w.cur], inc);
      steps_total += w.moves;
      walking = false;
    }
  }
  steps_total = wave_sum_u64(steps_total);
  if (lane == 0 && steps_total) atomic_add_u64(&ctr->walk_steps, steps_total);
}

// The weighted walk index (DESIGN.md §2 "Weighted walk index"): k_index_build's loop with the weighted walker.  A wave
// takes a contiguous range of index positions; a lane whose walk has stopped stores its terminal (internal id) and takes
// the range's next position (refill in ballot order).  Position p of node v is the weighted walk (seed, stream 0, v,
// p - off[v]) with the forced first hop: what k_w_walk_plan runs for walk p - off[v] of a residue entry v.  Only nodes
// with out-edges have positions.
__global__ __launch_bounds__(64) void k_w_index_build(const unsigned long long* __restrict__ off, uint32_t n,
                                                       unsigned long long total, WWalkGraph G,
                                                       const int32_t* __restrict__ new2old, double alpha, uint32_t k0,
                                                       uint32_t k1, int32_t* __restrict__ term,
                                                       unsigned long long* __restrict__ steps_out) {
  const int lane = threadIdx.x;
  const unsigned long long groups = (total + 63) / 64;
  const unsigned long long per = (groups + gridDim.x - 1) / gridDim.x * 64;
  const unsigned long long lo = (unsigned long long)blockIdx.x * per;
  if (lo >= total) return;
  const unsigned long long hi = lo + per < total ? lo + per : total;
  const uint32_t va = index_node_of(off, 0u, n - 1u, lo);
  const uint32_t vb = index_node_of(off, va, n - 1u, hi - 1ull);
  unsigned long long cursor = lo, pos = 0, steps = 0;
  WWalker w;
  bool walking = false;
  for (;;) {
    const unsigned long long need = __ballot(!walking);
    if (need && cursor < hi) {
      const unsigned long long avail = hi - cursor;
      const uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
      if (!walking && rank < avail) {
        pos = cursor + rank;
        const uint32_t v = index_node_of(off, va, vb, pos);
        const unsigned long long sext = G.out_ext[v];
        w_walker_init(w, (int32_t)v, sext, new2old[v], pos - off[v], 0u, true);
        if ((sext >> 32) == 0) term[pos] = (int32_t)v;  // (no node without out-edges has a position)
        else walking = true;
      }
      const unsigned long long want = __popcll(need);
      cursor += want < avail ? want : avail;
    }
    if (__ballot(walking) == 0) {
      if (cursor >= hi) break;
      continue;
    }
    if (walking && w_walker_step(w, G, alpha, k0, k1)) {
      term[pos] = w.cur;
      steps += w.moves;
      walking = false;
    }
  }
  steps = wave_sum_u64(steps);
  if (lane == 0 && steps) atomic_add_u64(steps_out, steps);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static WWalkGraph walk_graph(const GraphData* D) { return WWalkGraph{D->out_ext, D->out_ci, D->out_cum, D->wsum}; }

int launch_w_prepare(pprhip_graph* g, const PushArgs& a, int fbuf, uint32_t nf, bool scatter_dense, int cbuf, int dead_slot,
                     unsigned long long* next_counter) {
  const uint32_t grid = grid_for(nf, 256, 512);
  k_w_prepare<<<dim3(grid), dim3(256), 0, g->stream>>>(g->F[fbuf], nf, g->gr->out_ext, g->gr->wsum, g->residue, g->reserve,
                                                       g->cF, scatter_dense ? g->cdense[cbuf] : nullptr, g->ctr, dead_slot,
                                                       next_counter, a.alpha);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_w_push(pprhip_graph* g, const PushArgs& a, int fbuf, uint32_t nf, uint64_t ef, int dead_slot,
                  unsigned long long* next_counter) {
  const uint32_t grid = grid_for(ef, kWTile, 2048);
  k_w_push<<<dim3(grid), dim3(256), 0, g->stream>>>(g->F[fbuf], g->cF, g->eoff[fbuf], nf, (unsigned long long)ef,
                                                    g->gr->out_ext, g->gr->out_ci, g->gr->out_w, g->residue, g->F[fbuf ^ 1],
                                                    g->eoff[fbuf ^ 1], g->ctr, dead_slot, next_counter, a.src, a.rmax);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_w_dense_level(pprhip_graph* g, const PushArgs& a, int cbuf, int out_slot, int dead_slot) {
  const GraphData* D = g->gr;
  // a source without in-edges still receives returned dead-end mass: one extra apply thread (a seed set: one per live
  // seed without in-edges, and the live seeds' landing weights go to the apply kernel)
  const SeedTable* sd = (g->seed_on && a.mode != kPower) ? g->seeds : nullptr;
  const int src_extra = sd ? (int)sd->n_zin : (a.src >= 0 && D->h_in_rp[a.src + 1] == D->h_in_rp[a.src]) ? 1 : 0;
  if (D->n_chunks) {
    constexpr uint32_t kWaves = 8;  // per workgroup of 512 threads
    const uint32_t want = (D->n_chunks + kWaves - 1) / kWaves;
    const uint32_t grid = std::min<uint32_t>(want, (uint32_t)D->n_cus * 4u);
    k_w_dense_edges<<<dim3(grid), dim3(64 * kWaves), 0, g->stream>>>(D->in_ci, D->in_w, D->start_flags, D->chunk_starts,
                                                                    D->n_chunks, g->cdense[cbuf], g->acc_nz);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  const uint32_t rows = D->n_nz + (uint32_t)src_extra;
  const uint32_t grid = (rows + 255) / 256;
  if (grid) {
    const auto apply = a.mode == kPower ? &k_w_dense_apply<true, false>
                       : sd             ? &k_w_dense_apply<false, true>
                                        : &k_w_dense_apply<false, false>;
    apply<<<dim3(grid), dim3(256), 0, g->stream>>>(D->nz_rows, D->n_nz, g->acc_nz, D->out_ext, D->wsum, g->cdense[cbuf ^ 1],
                                                   g->residue, g->reserve, g->ctr, g->blk_pack, g->blk_dead, g->blk_ndead,
                                                   dead_slot, src_extra, a.src, a.alpha, a.rmax, sd ? sd->w_node : nullptr,
                                                   sd ? sd->zin : nullptr);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  if (sd) PPRHIP_TRY(launch_wq_land_dense(g, dead_slot));
  return reduce_partials(g, grid, out_slot, dead_slot ^ 1, true);
}

int launch_w_walk_batch(pprhip_graph* g, const int32_t* d_starts, const uint64_t* d_idx, uint64_t count, double alpha,
                        uint64_t seed, uint32_t stream, int no_zero_hop, int32_t* d_term, uint32_t* d_steps) {
  if (count == 0) return PPRHIP_OK;
  const uint64_t b = (count + 255) / 256;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(b, (uint64_t)g->gr->n_cus * 4u);
  k_w_walk_batch<<<dim3(grid), dim3(256), 0, g->stream>>>(d_starts, (const unsigned long long*)d_idx,
                                                          (unsigned long long)count, walk_graph(g->gr), g->gr->new2old, alpha,
                                                          (uint32_t)seed, (uint32_t)(seed >> 32), stream, no_zero_hop, d_term,
                                                          d_steps);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_w_walk_run(pprhip_graph* g, double alpha, uint64_t seed, double* target, uint32_t stream, bool no_zero_hop) {
  // a fixed grid of waves, each with an equal share of whatever the plan holds; the host's bound of the walk count
  // (g->walk_hint) only trims the grid of a short phase (kernels_walk.hip: mc_walk_grid)
  uint32_t grid = (uint32_t)g->gr->n_cus * 16u;
  if (g->walk_hint) grid = (uint32_t)std::min<unsigned long long>(grid, std::max<unsigned long long>((g->walk_hint + 63) / 64, 1ull));
  g->walk_hint = 0;
  const WalkPlanRec* rec = (g->mc_plan_rec2 && (g->mc_last_plan & 1u)) ? g->mc_plan_rec2 : g->mc_plan_rec;
  const int cell = (int)(g->mc_last_plan % 3u);
  // Whole-graph weighted FORA walks (stream 0, forced first hop, walk indices 0 .. omega_i - 1 per residue node; their
  // plan is k_mc_plan<0>, which clears ctr->walks_over) are read from the handle's weighted walk index when it was built
  // at this alpha and seed, bit for bit: the serve kernel on the same grid, then the walker for what the index does not
  // hold.  Everything else - the top-k rounds among it (stream = round, no forced hop) - walks.
  const WalkIndex* ix = g->gr->widx_w;
  if (ix && stream == 0u && no_zero_hop && std::memcmp(&ix->alpha, &alpha, sizeof alpha) == 0 && ix->seed == seed) {
    PPRHIP_TRY(launch_index_serve(g, ix, target, grid));
    k_w_walk_plan<true><<<dim3(grid), dim3(64), 0, g->stream>>>(rec, walk_graph(g->gr), target, alpha, (uint32_t)seed,
                                                                (uint32_t)(seed >> 32), 0u, 1, g->ctr, cell,
                                                                (const unsigned long long*)ix->off);
  } else {
    k_w_walk_plan<false><<<dim3(grid), dim3(64), 0, g->stream>>>(rec, walk_graph(g->gr), target, alpha, (uint32_t)seed,
                                                                 (uint32_t)(seed >> 32), stream, no_zero_hop ? 1 : 0, g->ctr,
                                                                 cell, WNoIndex{});
  }
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_w_index_build(pprhip_graph* g, const TerminalTable* ix, unsigned long long* d_steps) {
  if (ix->total == 0) return PPRHIP_OK;
  const uint64_t cap = (uint64_t)g->gr->n_cus * 16u;  // launch_w_walk_run's waves
  const uint64_t groups = (ix->total + 63) / 64;
  const uint32_t grid = (uint32_t)(groups < cap ? groups : cap);
  k_w_index_build<<<dim3(grid), dim3(64), 0, g->stream>>>(ix->off, g->gr->n, (unsigned long long)ix->total,
                                                          walk_graph(g->gr), g->gr->new2old, ix->alpha,
                                                          (uint32_t)ix->seed, (uint32_t)(ix->seed >> 32), ix->term, d_steps);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int init_kernels_weighted() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_w_push)));
  return PPRHIP_OK;
}

}  // namespace pprhip
