// kernels_walk.hip — Monte-Carlo refinement: one random walk per lane with refill (gfx950).
//
// Replaces Monte_Carlo.random_walk / random_walk_no_zero_hop (Monte_Carlo.java:60-133) and the
// walk loops of Fora_Whole_Graph.java:119-140 / Fora_Topk.java:155-168.  The reference draws from
// an unseeded ThreadLocalRandom; here walk (seed, stream, start, walk_idx) is a pure function of
// its counter: Philox4x32-10 with key = seed and counter = (start, idx_lo, idx_hi16 | stream<<16,
// block).  Decision k of a walk uses block k>>1, words 2(k&1) (stop test: word * 2^-32 < alpha)
// and 2(k&1)+1 (neighbour pick: (word * degree) >> 32).  The CPU oracle restates the same
// function, so terminals can be compared walk by walk.
//
// Memory-bound random gathers (one packed row extent + one col_idx per step); no MFMA.
#include <algorithm>

#include "device_utils.hpp"
#include "engine.hpp"

namespace pprhip {

struct Philox {
  uint32_t x[4];
};

__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
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
  Philox p;
  p.x[0] = c0; p.x[1] = c1; p.x[2] = c2; p.x[3] = c3;
  return p;
}

// Per-lane walk state machine: one decision per call of step().
struct Walker {
  int32_t start, cur;
  uint32_t c0, c1, c2;  // counter words 0-2 (original id of the start node, walk index, stream)
  uint32_t k;          // next decision number
  uint32_t w_stop, w_pick, w_stop2, w_pick2;  // cached Philox block
  uint32_t moves;
  bool forced;         // the next decision is the forced first hop (no_zero_hop)
  uint32_t b, d;       // out-row of the current node: first edge, degree
  uint32_t sb, sd;     // the same for the start node
};

__device__ __forceinline__ void walker_init(Walker& w, int32_t start, unsigned long long start_ext, int32_t start_orig,
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

// Returns true when the walk has stopped (w.cur is the terminal).
// A step reads one 16-byte edge record {neighbour, the neighbour's first out-edge, its out-degree}: the row extent
// the *next* step needs comes with the neighbour's id, so a step costs one random line instead of two (the extent
// array was the second: 0.24 lines per step beyond L2 on R-MAT 22).
__device__ __forceinline__ bool walker_step(Walker& w, const uint4* __restrict__ walk_rec, double alpha, uint32_t k0,
                                            uint32_t k1) {
  uint32_t ws, wp;
  if ((w.k & 1u) == 0) {
    const Philox p = philox4x32_10(w.c0, w.c1, w.c2, w.k >> 1, k0, k1);
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
    if ((double)ws * (1.0 / 4294967296.0) < alpha) return true;  // Monte_Carlo.java:76-78
  }
  w.forced = false;
  if (w.d > 0) {
    const uint4 r = walk_rec[w.b + (uint32_t)(((unsigned long long)wp * w.d) >> 32)];  // :81-86
    w.cur = (int32_t)r.x;
    w.b = r.y;
    w.d = r.z;
  } else {  // :87-90 dead end: restart at the walk's start node
    w.cur = w.start;
    w.b = w.sb;
    w.d = w.sd;
  }
  w.moves++;
  return false;
}

// ------------------------------------------------------------------------------------------------
// walk plan: one entry per residue node, walk ranges as an exclusive prefix over entries
// ------------------------------------------------------------------------------------------------
// walks a residue entry starts, and the increment each of them carries
template <int VARIANT>
__device__ __forceinline__ bool plan_entry(double r, double alpha, double rsum, double nrw, unsigned long long* omega_i,
                                           double* incr) {
  if (!(r > 0.0) || !(nrw > 0.0)) return false;
  if (VARIANT == 0) {  // Fora_Whole_Graph.java:123,129-131
    if (!(rsum > 0.0)) return false;
    r *= (1.0 - alpha);
    const double x = r / rsum * nrw;
    *omega_i = (unsigned long long)ceil(x);
    const double a_i = x / (double)*omega_i;
    *incr = a_i / nrw * rsum;
  } else {  // Fora_Topk.java:157-159
    const double x = r * nrw;
    *omega_i = (unsigned long long)ceil(x);
    const double a_i = x / (double)*omega_i;
    *incr = a_i / nrw;
  }
  return *omega_i > 0;
}

template <int VARIANT>
__global__ __launch_bounds__(256) void k_mc_plan(uint32_t n, const double* __restrict__ res, double* __restrict__ target,
                                                  double alpha, double rsum, double nrw, double omega_dev,
                                                  const unsigned long long* __restrict__ out_ext,
                                                  const int32_t* __restrict__ new2old, WalkPlanRec* __restrict__ plan,
                                                  DevCounters* ctr, int parity, int next_cell,
                                                  const double* __restrict__ copy_src, double* __restrict__ copy_dst) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctr->mc_plan[next_cell] = 0ull;  // (engine.hpp: DevCounters::mc_plan)
    if (VARIANT == 0) ctr->walks_over = 0ull;  // (counted anew by the k_index_serve of this phase, if one runs)
  }
  const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
  const uint32_t lo = blockIdx.x * per;
  const uint32_t hi = lo + per < n ? lo + per : n;
  if (lo >= hi) return;
  if (omega_dev > 0.0) {
    // the budget from the residue sum on the device, with the host's own expressions (Fora_Topk.java:148,151 /
    // Fora_Whole_Graph.java:112-113): rsum = sum * (1 - alpha); nrw = (long long)(omega * rsum)
    if (blockIdx.x == 0 && threadIdx.x == 0) ctr->plan_sum[parity] = ctr->sum_out;  // for the round's selection header
    rsum = ctr->sum_out * (1.0 - alpha);
    const double nrw_d = omega_dev * rsum;
    nrw = (nrw_d == nrw_d && nrw_d > 0.0) ? (double)(long long)nrw_d : 0.0;
  }
  block_range_compact(
      lo, hi, &ctr->mc_plan[parity],
      [&](uint32_t v, unsigned long long* w) {
        double incr;
        return plan_entry<VARIANT>(res[v], alpha, rsum, nrw, w, &incr);
      },
      [&](uint32_t v, uint32_t pos, unsigned long long woff, unsigned long long) {
        unsigned long long w;
        WalkPlanRec r;
        r.inc = 0.0;
        (void)plan_entry<VARIANT>(res[v], alpha, rsum, nrw, &w, &r.inc);
        r.woff = woff;
        r.ext = out_ext[v];  // what a walk needs of its start node travels with the entry: the walk kernel reads
        r.node = (int32_t)v;  // entries as a stream and nothing else before a walk's first step
        r.orig = new2old[v];
        plan[pos] = r;
      });
  if (VARIANT == 0) {  // Fora_Whole_Graph.java:122,124-127: every residue entry credits alpha * r to its own reserve
    for (uint32_t v = lo + threadIdx.x; v < hi; v += 256) {
      const double r = res[v];
      if (r > 0.0) target[v] = target[v] + r * alpha;
    }
  }
  // top-k rounds: the estimate the walks add to starts as a copy of the push reserve (Fora_Topk.java:143) - taken here,
  // in the pass that reads the same range anyway, when the caller has no use for the old estimate any more
  if (copy_dst)
    for (uint32_t v = lo + threadIdx.x; v < hi; v += 256) copy_dst[v] = copy_src[v];
}

// k_mc_plan<1> with the device-side budget, in one pass (round 5; top-k rounds, Fora_Topk.java:148-159).  What the
// two-pass kernel did in 44 us for 2 M nodes - and the two sum kernels in front of it in 20 - happens here per tile of
// 2048 consecutive nodes, 8 per thread: every workgroup first adds up the `np` partial sums k_sum_partial has left (the
// same additions in the same order in every workgroup, so all of them derive the same budget; no k_sum_final launch),
// then a thread loads its 8 residues (and 8 reserves, when the estimate is to start as their copy: 16-byte loads),
// evaluates its entries once, and the tile is compacted with one workgroup scan and one packed atomic.
constexpr int kPlanItems = 8;
__global__ __launch_bounds__(256) void k_mc_plan_topk(uint32_t n, const double* __restrict__ res, double alpha,
                                                       double omega_dev, const double* __restrict__ partial, uint32_t np,
                                                       const unsigned long long* __restrict__ out_ext,
                                                       const int32_t* __restrict__ new2old, WalkPlanRec* __restrict__ plan,
                                                       DevCounters* ctr, int parity, int next_cell,
                                                       const double* __restrict__ copy_src, double* __restrict__ copy_dst) {
  __shared__ double s_red[4];
  __shared__ double s_sum;
  if (blockIdx.x == 0 && threadIdx.x == 0) ctr->mc_plan[next_cell] = 0ull;  // (engine.hpp: DevCounters::mc_plan)
  {
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < np; i += 256) acc += partial[i];
    const double sum = block_sum_f64(acc, s_red);
    if (threadIdx.x == 0) s_sum = sum;
    __syncthreads();
  }
  const double sum = s_sum;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctr->sum_out = sum;
    ctr->plan_sum[parity] = sum;  // for the round's selection header
  }
  // the budget with the host's own expressions: rsum = sum * (1 - alpha); nrw = (long long)(omega * rsum)
  const double rsum = sum * (1.0 - alpha);
  const double nrw_d = omega_dev * rsum;
  const double nrw = (nrw_d == nrw_d && nrw_d > 0.0) ? (double)(long long)nrw_d : 0.0;
  const uint32_t tile = 256u * kPlanItems;
  const uint32_t n_tiles = (n + tile - 1) / tile;
  for (uint32_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const uint32_t v0 = tl * tile + threadIdx.x * kPlanItems;
    double r[kPlanItems];
    if (v0 + kPlanItems <= n) {
      const double2* r2 = reinterpret_cast<const double2*>(res + v0);
#pragma unroll
      for (int i = 0; i < kPlanItems / 2; ++i) {
        const double2 x = r2[i];
        r[2 * i] = x.x;
        r[2 * i + 1] = x.y;
      }
      if (copy_dst) {
        const double2* s2 = reinterpret_cast<const double2*>(copy_src + v0);
        double2* d2 = reinterpret_cast<double2*>(copy_dst + v0);
        double2 y[kPlanItems / 2];
#pragma unroll
        for (int i = 0; i < kPlanItems / 2; ++i) y[i] = s2[i];
#pragma unroll
        for (int i = 0; i < kPlanItems / 2; ++i) d2[i] = y[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < kPlanItems; ++i) {
        r[i] = v0 + i < n ? res[v0 + i] : 0.0;
        if (copy_dst && v0 + i < n) copy_dst[v0 + i] = copy_src[v0 + i];
      }
    }
    bool take[kPlanItems];
    unsigned long long w[kPlanItems];
    double inc[kPlanItems];
#pragma unroll
    for (int i = 0; i < kPlanItems; ++i) {
      w[i] = 0;
      inc[i] = 0.0;
      take[i] = plan_entry<1>(r[i], alpha, rsum, nrw, &w[i], &inc[i]);
    }
    block_tile_compact<kPlanItems>(take, w, &ctr->mc_plan[parity], [&](int i, uint32_t pos, unsigned long long woff) {
      const uint32_t v = v0 + (uint32_t)i;
      WalkPlanRec rec;
      rec.inc = inc[i];
      rec.woff = woff;
      rec.ext = out_ext[v];
      rec.node = (int32_t)v;
      rec.orig = new2old[v];
      plan[pos] = rec;
    });
  }
}

// ------------------------------------------------------------------------------------------------
// walk kernel: one wave per workgroup, each with a contiguous share of the phase's walks.  A lane whose walk has
// stopped takes the wave's next walk at once, so lanes stay busy although walk lengths are geometric, and the wave only
// drains once, at the end of its share (with a workgroup per 1024 walks, as in round 2, every chunk ended in a tail
// of ~20 steps with few lanes walking: 36 G steps/s).  The entries of the next kWalkWindow walks are staged in LDS (a window);
// a refill reads LDS only.
// Round 4, tried and taken back: "every load carries a full wave".  A decision that issues no gather - the walk stops
// (alpha), or it stands on a dead end and restarts (52 % of R-MAT 22's nodes have no out-edge) - costs its lane the
// whole trip of the loop below, so a wave's load carries 42 of 64 lanes.  A form of the loop in which lanes take
// decisions (stop -> deposit -> next walk -> first decision; dead end -> restart -> next decision) until every lane
// holds a gather, and only then the wave loads, carried 60.4 lanes per load (counters walk_loads / walk_lanes) and ran
// at the SAME rate one query at a time (39.0 G steps/s, 2.54 ms per query against 2.6) and slower beside the sweeps,
// where a walk kernel has four waves per CU and three to four decision rounds per load are not hidden (24.5 against
// ~33 G steps/s, headline 312 against 329 queries/s): the rate is what the memory system gives this address stream,
// not a matter of how full the loads are (gpurun_out/r04b_bench.json).
// The queries of a batched call draw the same walks (one seed, stream 0): k_mc_walk<kWalkShared> reads a walk's terminal
// from the call's cache when an earlier query has walked it - 4 bytes streamed and the deposit, no Philox, no record -
// and 98.8 % of a 128-query call's walks on R-MAT 22 are served so: 713 us per query beside the sweeps against 1 124,
// 0.163 ns per walk, which is the terminals' fp64 atomics (profiles/walk_share_ab.txt).
// ------------------------------------------------------------------------------------------------
constexpr int kWalkWindow = 128;
constexpr uint32_t kWalkWavesBeside = 4;   // ... of a walk kernel that runs beside other queries' kernels
constexpr uint32_t kWalkWavesPerCu = 16;  // 4.3 KB of LDS each: room for another stream's workgroups on the CU

struct WalkWindow {  // LDS, one per wave
  unsigned long long woff[kWalkWindow + 1];
  unsigned long long ext[kWalkWindow];
  double inc[kWalkWindow];
  int32_t node[kWalkWindow];
  int32_t orig[kWalkWindow];
  uint8_t ent[kWalkWindow];  // staged entry of every walk of the window
};

// first entry whose walk range starts beyond walk x (woff[0] = 0, so >= 1), 64 probes per round
__device__ __forceinline__ uint32_t plan_upper_bound(const WalkPlanRec* __restrict__ plan, uint32_t n_src,
                                                     unsigned long long x, int lane) {
  uint32_t a = 0, b = n_src;  // the answer lies in [a, b]
  while (a < b) {
    const uint32_t step = (b - a + 63u) / 64u;
    const unsigned long long idx = (unsigned long long)a + (unsigned long long)lane * step;
    const bool gt = idx >= b || plan[idx].woff > x;
    const unsigned long long mask = __ballot(gt);
    if (mask == 0) {  // all 64 probes <= x
      a = (uint32_t)std::min<unsigned long long>((unsigned long long)a + 63ull * step + 1ull, b);
      continue;
    }
    const uint32_t f = (uint32_t)__builtin_ctzll(mask);
    const unsigned long long nb = (unsigned long long)a + (unsigned long long)f * step;
    if (f > 0) a = a + (f - 1u) * step + 1u;
    b = (uint32_t)std::min<unsigned long long>(nb, b);
    if (f == 0) b = a;
  }
  return a;
}

// INDEXED (idx_off: the walk index's offsets): k_index_serve has deposited the stored terminals of this plan; a walk
// whose index lies below its node's capacity is skipped here (a fourth early-out beside the dead-end start), the others
// - an entry's tail [cap, omega_i), every walk of a dead-end start - run with their own indices.  The unindexed
// instantiation is the kernel as it was.
// SHARED (idx_off: the offsets of the call's terminal cache, engine.hpp: WalkShare): a lane that takes walk (v, j) with
// j < cap(v) first reads the walk's cell - the plan is in node order, so the lanes of a refill read consecutive cells: a
// streamed 4 bytes per walk.  A filled cell is the terminal an earlier query of the call (or another wave of this one)
// reached with the same counter and key: the lane deposits there and takes the next walk, at the cost of the probe and
// the deposit instead of ~6.7 gathered lines.  An empty cell: the walk runs as ever and stores its terminal with a
// plain 4-byte store when it stops.  Nothing orders the store against other kernels' probes and nothing needs to: a
// cell only goes from empty to the one value every writer writes, and a reader that still sees "empty" walks.  What
// bounds a phase that is mostly served is its deposits: fp64 atomics on the terminals, the hubs among them hot - which is
// why a large phase of a batched call leaves records instead ("deposits by tile" below).
enum WalkMode : int { kWalkPlain = 0, kWalkIndexed = 1, kWalkShared = 2 };
// What a walk does with its increment: the fp64 atomic at the terminal; a record (terminal, increment) at the walk's own
// index for the kernels under "deposits by tile" below, when the phase has dep.min_walks walks or more - a device-uniform
// test on the plan's count that those kernels repeat - and the index lies below dep.cap (the others add atomically, in
// the same phase); or nothing (libpprhip_hooks.so's measurement of what the deposits cost: the masses are wrong then).
// Walk gidx is taken by one lane of one wave and deposits once, so positions [0, min(walks, cap)) are all written, the
// lanes of a refill write consecutive ones, and no counter is needed.
enum WalkDepositMode : int { kDepAtomic = 0, kDepBinned = 1, kDepNone = 2 };
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;  // (dep.cap < 2^31)
template <int MODE>
__global__ __launch_bounds__(64) void k_mc_walk(const WalkPlanRec* __restrict__ plan_rec,
                                                 const uint4* __restrict__ walk_rec, double* __restrict__ target,
                                                 double alpha, uint32_t k0, uint32_t k1, uint32_t stream,
                                                 int no_zero_hop, DevCounters* ctr, int parity,
                                                 const unsigned long long* __restrict__ idx_off,
                                                 uint32_t* share_term, uint32_t n_nodes,
                                                 unsigned long long* __restrict__ share_usage, int dep_mode,
                                                 uint32_t* __restrict__ dep_key, double* __restrict__ dep_inc,
                                                 unsigned long long dep_cap, unsigned long long dep_min) {
  constexpr bool INDEXED = MODE == kWalkIndexed;
  constexpr bool SHARED = MODE == kWalkShared;
  constexpr unsigned long long kNoCell = ~0ull;
  // the plan kernel counted sources and walks into mc_plan[parity]; the query's totals grow by this phase
  const unsigned long long plan = ctr->mc_plan[parity];
  const uint32_t n_src = (uint32_t)(plan >> kPackShift);
  const unsigned long long n_walks = plan & kPackMask;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctr->walks_total += n_walks;
    ctr->sources_total += n_src;
  }
  if (INDEXED && ctr->walks_over == 0ull) return;  // the index held every walk of the phase
  const unsigned long long rec_cap = dep_mode == kDepBinned && n_walks >= dep_min ? dep_cap : 0ull;  // (wave-uniform)
  uint32_t slot = kNoSlot;  // where this lane's walk leaves its record (kNoSlot: it adds at the terminal)
  auto deposit = [&](uint32_t t, double x) {
    if (slot != kNoSlot) {
      dep_key[slot] = t;
      dep_inc[slot] = x;
    } else if (dep_mode != kDepNone) {
      atomic_add_noret(&target[t], x);
    }
  };
  __shared__ WalkWindow S;
  const int lane = threadIdx.x;
  // this wave's share: whole groups of 64 walks, so that a short phase still spreads over the grid
  const unsigned long long groups = (n_walks + 63) / 64;
  const unsigned long long per = (groups + gridDim.x - 1) / gridDim.x * 64;
  unsigned long long cursor = (unsigned long long)blockIdx.x * per;
  if (cursor >= n_walks) return;
  const unsigned long long w_hi = cursor + per < n_walks ? cursor + per : n_walks;
  uint32_t e = plan_upper_bound(plan_rec, n_src, cursor, lane) - 1u;  // the entry that holds walk `cursor`
  unsigned long long win_lo = cursor, win_end = cursor;
  unsigned long long steps_total = 0;
  Walker w;
  double inc = 0.0;
  bool walking = false;
  unsigned long long n_loads = 0, n_lanes = 0;  // (wave-uniform) loads issued, lanes they carried
  unsigned long long cell = kNoCell;            // SHARED: where this lane's walk leaves its terminal
  unsigned long long n_served = 0, n_stored = 0;
  for (;;) {
    const unsigned long long need = __ballot(!walking);
    if (need && cursor < w_hi) {
      if (cursor >= win_end) {
        // stage the entries of walks [cursor, cursor + kWalkWindow): at most that many from e, which holds walk `cursor`
        // (every entry owns >= 1 walk)
        win_lo = cursor;
        win_end = cursor + kWalkWindow < w_hi ? cursor + kWalkWindow : w_hi;
        __syncthreads();  // refills of the window before have read it
        WalkPlanRec r[kWalkWindow / 64];
#pragma unroll
        for (int q = 0; q < kWalkWindow / 64; ++q) {
          const unsigned long long idx = (unsigned long long)e + (unsigned long long)(q * 64 + lane);
          if (idx < n_src) {
            r[q] = plan_rec[idx];
          } else {
            r[q].woff = n_walks;
            r[q].inc = 0.0;
            r[q].ext = 0ull;
            r[q].node = 0;
            r[q].orig = 0;
          }
        }
        unsigned long long last = n_walks;
        if (lane == 0 && (unsigned long long)e + kWalkWindow < n_src) last = plan_rec[(size_t)e + kWalkWindow].woff;
#pragma unroll
        for (int q = 0; q < kWalkWindow / 64; ++q) S.ent[lane * (kWalkWindow / 64) + q] = 0;
#pragma unroll
        for (int q = 0; q < kWalkWindow / 64; ++q) {
          const int j = q * 64 + lane;
          S.woff[j] = r[q].woff;
          S.ext[j] = r[q].ext;
          S.inc[j] = r[q].inc;
          S.node[j] = r[q].node;
          S.orig[j] = r[q].orig;
        }
        if (lane == 0) S.woff[kWalkWindow] = last;
        __syncthreads();
        // entry j > 0 that starts inside the window marks its first walk; a running maximum spreads the marks
#pragma unroll
        for (int q = 0; q < kWalkWindow / 64; ++q) {
          const int j = q * 64 + lane;
          if (j > 0 && r[q].woff >= win_lo && r[q].woff < win_end) S.ent[r[q].woff - win_lo] = (uint8_t)j;
        }
        __syncthreads();
        constexpr int kPer = kWalkWindow / 64;  // positions per lane
        uint32_t m[kPer];
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
          m[q] = S.ent[lane * kPer + q];
          if (q > 0 && m[q] < m[q - 1]) m[q] = m[q - 1];
        }
        uint32_t run = m[kPer - 1];  // inclusive maximum over the lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t o = __shfl_up(run, d);
          if (lane >= d) run = run > o ? run : o;
        }
        uint32_t before = __shfl_up(run, 1);
        if (lane == 0) before = 0;
#pragma unroll
        for (int q = 0; q < kPer; ++q) S.ent[lane * kPer + q] = (uint8_t)(m[q] > before ? m[q] : before);
        __syncthreads();
      }
      const unsigned long long avail = win_end - cursor;
      const uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
      if (!walking && rank < avail) {
        const unsigned long long gidx = cursor + rank;
        const uint32_t j = S.ent[gidx - win_lo];
        const int32_t start = S.node[j];
        inc = S.inc[j];
        const unsigned long long sext = S.ext[j];
        const unsigned long long widx = gidx - S.woff[j];
        walker_init(w, start, sext, S.orig[j], widx, stream, no_zero_hop != 0);
        slot = gidx < rec_cap ? (uint32_t)gidx : kNoSlot;
        bool stored = false;
        if (INDEXED) stored = widx < idx_off[start + 1] - idx_off[start];
        if (stored) {  // k_index_serve has deposited this walk's terminal
        } else if ((sext >> 32) == 0) {
          deposit((uint32_t)start, inc);  // Monte_Carlo.java:70-72 / :106-108
        } else if (SHARED) {
          const unsigned long long o0 = idx_off[start];
          cell = widx < idx_off[start + 1] - o0 ? o0 + widx : kNoCell;
          const uint32_t t = cell != kNoCell ? share_term[cell] : kWalkShareEmpty;
          if (t < n_nodes) {  // (kWalkShareEmpty is no node)
            deposit(t, inc);
            n_served++;
          } else {
            walking = true;
          }
        } else {
          walking = true;
        }
      }
      const unsigned long long want = __popcll(need);
      cursor += want < avail ? want : avail;
      if (cursor >= win_end) {  // window used up: e becomes the entry of the next walk
        const uint32_t jl = S.ent[win_end - 1 - win_lo];
        e += S.woff[jl + 1] == win_end ? jl + 1u : jl;
      }
    }
    if (__ballot(walking) == 0) {
      if (cursor >= w_hi) break;
      continue;
    }
    const bool can_load = walking && w.d > 0;  // (a lane that neither stops nor stands on a dead end gathers)
    bool stopped = false;
    if (walking) {
      stopped = walker_step(w, walk_rec, alpha, k0, k1);
      if (stopped) {
        deposit((uint32_t)w.cur, inc);
        steps_total += w.moves;
        walking = false;
        if (SHARED && cell != kNoCell) {
          share_term[cell] = (uint32_t)w.cur;
          n_stored++;
        }
      }
    }
    const unsigned long long loaded = __ballot(can_load && !stopped);
    n_loads += loaded ? 1ull : 0ull;
    n_lanes += (unsigned long long)__popcll(loaded);
  }
  steps_total = wave_sum_u64(steps_total);
  if (lane == 0 && steps_total) atomic_add_u64(&ctr->walk_steps, steps_total);
  if (lane == 0 && n_loads) {
    atomic_add_u64(&ctr->walk_loads, n_loads);
    atomic_add_u64(&ctr->walk_lanes, n_lanes);
  }
  if (SHARED) {
    n_served = wave_sum_u64(n_served);
    n_stored = wave_sum_u64(n_stored);
    if (lane == 0 && n_served) {
      atomic_add_u64(&ctr->share_served, n_served);
      atomic_add_u64(&share_usage[0], n_served);
    }
    if (lane == 0 && n_stored) {
      atomic_add_u64(&ctr->share_stored, n_stored);
      atomic_add_u64(&share_usage[1], n_stored);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// deposits by tile (engine.hpp: WalkDeposit)
// What is left of a batched query's walk phase once the call's cache serves its walks is one fp64 atomic per walk at a
// terminal: 64 lanes in 64 different lines per wave-instruction, executed at the memory side, the hubs' addresses hot.
// Instead the walk kernel streams a 12-byte record per walk (above) and five kernels behind it on the same stream turn
// the records into the same sums: k_dep_count counts the records per tile of 1 << tile_shift consecutive ids,
// k_dep_items turns the counts into the tiles' runs and a table of work items (tile, slice of at most dep.slice
// records: the first tile of an R-MAT holds a third of all records), k_dep_bin and k_dep_tile move the records into
// their runs (order inside a run is free), and k_dep_sum adds an item's records into a tile of LDS and the tile to the
// vector: by load-add-store when the item owns its tile, by atomics whose lanes are consecutive addresses when it
// shares it.  The records move in two radix passes (dep_move) so that a store instruction's lanes write consecutive
// positions: storing a record straight at its tile's cursor put a wave's 64 lanes into up to 64 lines of each array,
// with 2 048 tiles x 2 arrays open per workgroup, which no cache merges.  k_dep_bin sorts a workgroup's share into the
// runs of coarse bins of dep.bin consecutive tiles (runs are in tile order: a bin's run is its tiles' runs on end),
// key/inc -> bkey/binc; k_dep_tile sorts a unit (bin, slice of the bin's run) into the bin's tile runs, bkey/binc ->
// key/inc, which are dead by then.
// Nothing is sized on the host: grids are fixed, every kernel reads the phase's walk count from the plan's cell as the
// walk kernel does, and all five return at once when the walk kernel kept its atomics.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long dep_records(const DepositArgs& a, const DevCounters* ctr, int parity) {
  const unsigned long long n_walks = ctr->mc_plan[parity] & kPackMask;
  if (n_walks < a.min_walks) return 0ull;
  return n_walks < a.cap ? n_walks : a.cap;
}

// this workgroup's share of the records: whole multiples of 256, so that a thread's loop is uniform per wave
__device__ __forceinline__ void dep_share(unsigned long long n_rec, uint32_t* lo, uint32_t* hi) {
  const unsigned long long per = ((n_rec + gridDim.x - 1) / gridDim.x + 255ull) / 256ull * 256ull;
  const unsigned long long a = (unsigned long long)blockIdx.x * per, b = a + per;
  *lo = (uint32_t)(a < n_rec ? a : n_rec);
  *hi = (uint32_t)(b < n_rec ? b : n_rec);
}

// Measurement switch of the hooks library (PPRHIP_WALK_DEPOSIT_SKIP, a.skip; 0 in the product): the named pass keeps
// its loads, histograms and index arithmetic and stores nothing.  `never` is a condition on the loaded value that no
// record meets: it keeps the compiler from dropping the loads with the store.
__device__ __forceinline__ bool dep_stores(const DepositArgs& a, uint32_t pass, bool never) {
  return a.skip != pass || never;
}

__device__ __forceinline__ uint32_t dep_tile_of(const DepositArgs& a, uint32_t key) {
  const uint32_t t = key >> a.tile_shift;
  return t < a.n_tiles ? t : a.n_tiles - 1u;  // (a terminal is a node: the clamp only keeps a wrong record inside LDS)
}

__device__ __forceinline__ void dep_count_share(const DepositArgs& a, uint32_t lo, uint32_t hi, uint32_t* hist) {
  for (uint32_t t = threadIdx.x; t < a.n_tiles; t += 256u) hist[t] = 0u;
  __syncthreads();
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 256u) atomicAdd(&hist[dep_tile_of(a, a.key[i])], 1u);
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_dep_count(DepositArgs a, const DevCounters* ctr, int parity) {
  const unsigned long long n_rec = dep_records(a, ctr, parity);
  if (n_rec == 0) return;
  __shared__ uint32_t hist[kDepMaxTiles];
  uint32_t lo, hi;
  dep_share(n_rec, &lo, &hi);
  if (lo >= hi) return;
  dep_count_share(a, lo, hi, hist);
  for (uint32_t t = threadIdx.x; t < a.n_tiles; t += 256u) {  // (a wave's lanes: consecutive counters)
    const uint32_t c = hist[t];
    if (c && dep_stores(a, kDepSkipCount, c == 0xFFFFFFFFu)) atomicAdd(&a.tile_cnt[t], c);
  }
}

// One workgroup: thread i takes the tiles [i * per, (i + 1) * per), so the runs and the items are in tile order.
__global__ __launch_bounds__(256) void k_dep_items(DepositArgs a, const DevCounters* ctr, int parity) {
  const unsigned long long n_rec = dep_records(a, ctr, parity);
  if (n_rec == 0) return;
  __shared__ uint32_t s_scan[4];
  __shared__ uint32_t s_bin[kDepMaxBins + 1];  // where every bin's run starts, and the end of the last
  const uint32_t per = (a.n_tiles + 255u) / 256u;
  const uint32_t t_lo = threadIdx.x * per < a.n_tiles ? threadIdx.x * per : a.n_tiles;
  const uint32_t t_hi = t_lo + per < a.n_tiles ? t_lo + per : a.n_tiles;
  uint32_t recs = 0, its = 0;
  for (uint32_t t = t_lo; t < t_hi; ++t) {
    const uint32_t c = a.tile_cnt[t];
    recs += c;
    its += (c + a.slice - 1u) / a.slice;
  }
  uint32_t recs_all, its_all;
  uint32_t base = block_excl_scan_256<uint32_t>(recs, s_scan, &recs_all);
  uint32_t ib = block_excl_scan_256<uint32_t>(its, s_scan, &its_all);
  for (uint32_t t = t_lo; t < t_hi; ++t) {
    const uint32_t c = a.tile_cnt[t];
    a.tile_cur[t] = base;
    if (t % a.bin == 0u) s_bin[t / a.bin] = base;  // a bin's run starts where its first tile's does
    a.tile_cnt[t] = 0u;  // for the next phase
    const uint32_t k_n = (c + a.slice - 1u) / a.slice;
    for (uint32_t k = 0; k < k_n; ++k) {
      const uint32_t first = k * a.slice;
      const uint32_t len = c - first < a.slice ? c - first : a.slice;
      if (ib + k < a.items_cap) a.items[ib + k] = make_uint4(t, base + first, len, k_n > 1u ? 1u : 0u);
    }
    base += c;
    ib += k_n;
  }
  // the bins' cursors and the units of k_dep_tile (bin, slice of at most a.slice records of its run), in bin order
  if (threadIdx.x == 0) s_bin[a.n_bins] = recs_all;
  __syncthreads();
  const uint32_t b = threadIdx.x;  // (n_bins <= kDepMaxBins = 256: a bin per thread)
  const uint32_t b_first = b < a.n_bins ? s_bin[b] : 0u;
  const uint32_t b_len = b < a.n_bins ? s_bin[b + 1u] - b_first : 0u;
  const uint32_t u_n = (b_len + a.slice - 1u) / a.slice;
  uint32_t units_all;
  const uint32_t ub = block_excl_scan_256<uint32_t>(u_n, s_scan, &units_all);
  if (b < a.n_bins) a.bin_cur[b] = b_first;
  for (uint32_t k = 0; k < u_n; ++k) {
    const uint32_t first = k * a.slice;
    const uint32_t len = b_len - first < a.slice ? b_len - first : a.slice;
    if (ub + k < a.units_cap) a.units[ub + k] = make_uint4(b, b_first + first, len, 0u);
  }
  if (threadIdx.x == 0) {
    a.bin_cur[a.n_bins] = units_all < a.units_cap ? units_all : a.units_cap;  // (units_cap >= n_bins + cap / slice)
    const unsigned long long n_walks = ctr->mc_plan[parity] & kPackMask;
    a.stat[0] = its_all < a.items_cap ? its_all : a.items_cap;  // (items_cap >= n_tiles + cap / slice: never short)
    a.stat[1] += 1ull;
    a.stat[2] += n_rec;
    a.stat[3] += n_walks - n_rec;
  }
}

// One radix pass of a workgroup over the records [lo, hi) of src: into the runs of n_cls <= 256 classes of dst, class
// = (tile - t0) / div, whose cursors are cur[].  The workgroup sorts kDepChunk records at a time by class in LDS (a
// rank from an LDS counter, a scan over the classes) and stores them from there: LDS position p of a class goes to its
// piece's cursor plus p's place in the class, so consecutive lanes write consecutive positions and a class's records
// leave as whole lines but for the piece's two ends.  WHOLE: the workgroup first counts all its records per class and
// reserves one piece per run (one atomic per class; k_dep_bin, where a chunk has some 32 records per bin and the pieces
// of one workgroup follow each other); otherwise every chunk reserves its own pieces (k_dep_tile: one atomic per tile
// and chunk, no second read of the keys).  27 KB of LDS.
struct DepMoveLds {
  uint32_t pos[kDepMaxBins];  // next position of every class's piece in dst
  uint32_t cnt[kDepMaxBins];  // of the chunk: records per class; then: dst position minus LDS position of the class
  uint32_t off[kDepMaxBins];  // of the chunk: where the class's records start in LDS
  uint32_t scan[4];
  uint32_t key[kDepChunk];
  double inc[kDepChunk];
};

__device__ __forceinline__ uint32_t dep_class_of(const DepositArgs& a, uint32_t key, uint32_t t0, uint32_t div,
                                                 uint32_t n_cls) {
  const uint32_t c = (dep_tile_of(a, key) - t0) / div;
  return c < n_cls ? c : n_cls - 1u;  // (never: the clamp only keeps a wrong record inside LDS)
}

template <bool WHOLE>
__device__ __forceinline__ void dep_move(const DepositArgs& a, const uint32_t* __restrict__ src_key,
                                         const double* __restrict__ src_inc, uint32_t* __restrict__ dst_key,
                                         double* __restrict__ dst_inc, uint32_t lo, uint32_t hi, uint32_t n_rec,
                                         uint32_t t0, uint32_t div, uint32_t n_cls, uint32_t* cur, DepMoveLds& s) {
  constexpr uint32_t kPer = kDepChunk / 256u;
  const uint32_t tid = threadIdx.x;
  if (WHOLE) {
    s.pos[tid] = 0u;
    __syncthreads();
    for (uint32_t i = lo + tid; i < hi; i += 256u) atomicAdd(&s.pos[dep_class_of(a, src_key[i], t0, div, n_cls)], 1u);
    __syncthreads();
    // this workgroup's piece of every run it has records for (thread c keeps the cursor of class c from here on)
    const uint32_t c = s.pos[tid];
    s.pos[tid] = tid < n_cls && c ? atomicAdd(&cur[tid], c) : 0u;
  }
  for (uint32_t c0 = lo; c0 < hi; c0 += kDepChunk) {
    s.cnt[tid] = 0u;
    __syncthreads();
    uint32_t key[kPer], at[kPer];  // at: class << 16 | rank among the chunk's records of the class
    double x[kPer];
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t i = c0 + k * 256u + tid;
      key[k] = i < hi ? src_key[i] : 0u;
      x[k] = i < hi ? src_inc[i] : 0.0;
    }
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t cls = dep_class_of(a, key[k], t0, div, n_cls);
      if (c0 + k * 256u + tid < hi) at[k] = cls << 16 | atomicAdd(&s.cnt[cls], 1u);
    }
    __syncthreads();
    const uint32_t mine = s.cnt[tid];
    uint32_t total;
    const uint32_t off = block_excl_scan_256<uint32_t>(mine, s.scan, &total);
    uint32_t piece;
    if (WHOLE) {
      piece = s.pos[tid];
      s.pos[tid] = piece + mine;
    } else {
      piece = tid < n_cls && mine ? atomicAdd(&cur[tid], mine) : 0u;
    }
    s.off[tid] = off;
    s.cnt[tid] = piece - off;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k)
      if (c0 + k * 256u + tid < hi) {
        const uint32_t p = s.off[at[k] >> 16] + (at[k] & 0xFFFFu);
        if (p < kDepChunk) {  // (always: the ranks and the scan count the same records)
          s.key[p] = key[k];
          s.inc[p] = x[k];
        }
      }
    __syncthreads();
    for (uint32_t p = tid; p < total; p += 256u) {
      const uint32_t k = s.key[p];
      const double y = s.inc[p];
      const uint32_t dst = s.cnt[dep_class_of(a, k, t0, div, n_cls)] + p;
      if (dst < n_rec && dep_stores(a, kDepSkipScatter, y < -1e300)) {
        dst_key[dst] = k;
        dst_inc[dst] = y;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_dep_bin(DepositArgs a, const DevCounters* ctr, int parity) {
  const unsigned long long n_rec = dep_records(a, ctr, parity);
  if (n_rec == 0) return;
  __shared__ DepMoveLds s;
  uint32_t lo, hi;
  dep_share(n_rec, &lo, &hi);
  if (lo >= hi) return;
  dep_move<true>(a, a.key, a.inc, a.bkey, a.binc, lo, hi, (uint32_t)n_rec, 0u, a.bin, a.n_bins, a.bin_cur, s);
}

__global__ __launch_bounds__(256) void k_dep_tile(DepositArgs a, const DevCounters* ctr, int parity) {
  const unsigned long long n_rec = dep_records(a, ctr, parity);
  if (n_rec == 0) return;
  __shared__ DepMoveLds s;
  const uint32_t n_units = a.bin_cur[a.n_bins];
  for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const uint4 unit = a.units[u];
    const uint32_t t0 = unit.x * a.bin;
    if (t0 >= a.n_tiles || unit.y >= n_rec) continue;  // (never: the units cover the bins' runs)
    const uint32_t n_cls = a.n_tiles - t0 < a.bin ? a.n_tiles - t0 : a.bin;
    const uint32_t hi = unit.z < (uint32_t)n_rec - unit.y ? unit.y + unit.z : (uint32_t)n_rec;
    dep_move<false>(a, a.bkey, a.binc, a.key, a.inc, unit.y, hi, (uint32_t)n_rec, t0, 1u, n_cls, a.tile_cur + t0, s);
  }
}

__global__ __launch_bounds__(256) void k_dep_sum(DepositArgs a, const DevCounters* ctr, int parity,
                                                  double* __restrict__ target) {
  const unsigned long long n_rec = dep_records(a, ctr, parity);
  if (n_rec == 0) return;
  __shared__ double acc[1u << kDepTileShift];
  const uint32_t n_items = (uint32_t)a.stat[0];
  const uint32_t width = 1u << a.tile_shift;
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const uint4 item = a.items[it];
    const uint32_t v0 = item.x << a.tile_shift;
    for (uint32_t j = threadIdx.x; j < width; j += 256u) acc[j] = 0.0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < item.z; i += 256u) {
      const unsigned long long p = (unsigned long long)item.y + i;
      if (p >= n_rec) break;  // (never: the items cover the runs)
      const uint32_t off = a.key[p] - v0;
      if (off < width) (void)__hip_atomic_fetch_add(&acc[off], a.inc[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < width; j += 256u) {
      const double x = acc[j];
      const uint32_t v = v0 + j;
      if (x != 0.0 && v < a.n && dep_stores(a, kDepSkipSum, x < -1e300)) {
        if (item.w) atomic_add_noret(&target[v], x);
        else target[v] = target[v] + x;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// walk index (FORA+, DESIGN.md §2 "Walk index"): build and serve
// ------------------------------------------------------------------------------------------------
// (index_node_of, the node of an index position, is in device_utils.hpp: k_w_index_build shares it)
// A wave takes a contiguous range of index positions; a lane whose walk has stopped stores its terminal (internal id)
// and takes the range's next position (refill in ballot order, as k_pair_walk).  Position p of node v is walk
// (seed, stream 0, v, p - off[v]) with the forced first hop: what k_mc_walk would run for walk p - off[v] of a residue
// entry v.  Only nodes with out-edges have positions.
__global__ __launch_bounds__(64) void k_index_build(const unsigned long long* __restrict__ off, uint32_t n,
                                                     unsigned long long total,
                                                     const unsigned long long* __restrict__ out_ext,
                                                     const uint4* __restrict__ walk_rec,
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
  Walker w;
  bool walking = false;
  for (;;) {
    const unsigned long long need = __ballot(!walking);
    if (need && cursor < hi) {
      const unsigned long long avail = hi - cursor;
      const uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
      if (!walking && rank < avail) {
        pos = cursor + rank;
        const uint32_t v = index_node_of(off, va, vb, pos);
        const unsigned long long sext = out_ext[v];
        walker_init(w, (int32_t)v, sext, new2old[v], pos - off[v], 0u, true);
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
    if (walking && walker_step(w, walk_rec, alpha, k0, k1)) {
      term[pos] = w.cur;
      steps += w.moves;
      walking = false;
    }
  }
  steps = wave_sum_u64(steps);
  if (lane == 0 && steps) atomic_add_u64(steps_out, steps);
}

// The walks of a plan (the WalkPlanRec stream k_mc_plan<0> wrote) from the index: a wave has a contiguous share of the
// phase's walks, as in k_mc_walk, and takes it 64 walks at a time - lane l the walk c + l.  The entries those walks
// belong to are at most 64 from the entry of walk c on (every entry owns a walk): their walk offsets, increments and
// nodes are staged in LDS, a lane finds its entry there, and walk i of node v reads term[off[v] + i] - consecutive
// lanes inside an entry read consecutive terminals - and adds the entry's increment there.  No Philox, no edge record.
// A walk the index does not hold (i >= cap(v); every walk of a dead-end start, whose capacity is 0) is counted in
// ctr->walks_over and left to k_mc_walk<kWalkIndexed>.
struct ServeWindow {  // LDS, one per wave
  unsigned long long woff[65];
  double inc[64];
  int32_t node[64];
};

__global__ __launch_bounds__(64) void k_index_serve(const WalkPlanRec* __restrict__ plan_rec,
                                                     const unsigned long long* __restrict__ idx_off,
                                                     const int32_t* __restrict__ idx_term, double* __restrict__ target,
                                                     DevCounters* ctr, int parity,
                                                     unsigned long long* __restrict__ usage) {
  const unsigned long long plan = ctr->mc_plan[parity];
  const uint32_t n_src = (uint32_t)(plan >> kPackShift);
  const unsigned long long n_walks = plan & kPackMask;
  __shared__ ServeWindow S;
  const int lane = threadIdx.x;
  const unsigned long long groups = (n_walks + 63) / 64;
  const unsigned long long per = (groups + gridDim.x - 1) / gridDim.x * 64;
  const unsigned long long lo = (unsigned long long)blockIdx.x * per;
  if (lo >= n_walks) return;
  const unsigned long long hi = lo + per < n_walks ? lo + per : n_walks;
  uint32_t e = plan_upper_bound(plan_rec, n_src, lo, lane) - 1u;  // the entry that holds walk `lo`
  unsigned long long served = 0, over = 0;
  for (unsigned long long c = lo; c < hi; c += 64) {
    __syncthreads();  // the chunk before has read the window
    const unsigned long long ei = (unsigned long long)e + (unsigned long long)lane;
    if (ei < n_src) {
      const WalkPlanRec r = plan_rec[ei];
      S.woff[lane] = r.woff;
      S.inc[lane] = r.inc;
      S.node[lane] = r.node;
    } else {
      S.woff[lane] = n_walks;
      S.inc[lane] = 0.0;
      S.node[lane] = 0;
    }
    if (lane == 0) S.woff[64] = (unsigned long long)e + 64ull < n_src ? plan_rec[(size_t)e + 64].woff : n_walks;
    __syncthreads();
    const unsigned long long gw = c + (unsigned long long)lane;
    const unsigned long long gq = gw < hi ? gw : hi - 1ull;
    uint32_t j = 0;  // the largest staged entry whose first walk is <= gq (woff[0] <= c: e holds walk c)
#pragma unroll
    for (uint32_t step = 32; step > 0; step >>= 1)
      if (S.woff[j + step] <= gq) j += step;
    if (gw < hi) {
      const int32_t v = S.node[j];
      const unsigned long long i = gw - S.woff[j];
      const unsigned long long o0 = idx_off[v], o1 = idx_off[v + 1];
      if (i < o1 - o0) {
        atomic_add_noret(&target[idx_term[o0 + i]], S.inc[j]);
        served++;
      } else {
        over++;
      }
    }
    // e becomes the entry of walk c + 64: lane 63's entry, or the one behind it when that starts there
    const uint32_t jl = (uint32_t)__shfl((int)j, 63);
    e += S.woff[jl + 1] == c + 64ull ? jl + 1u : jl;
  }
  served = wave_sum_u64(served);
  over = wave_sum_u64(over);
  if (lane == 0) {
    if (served) {
      atomic_add_u64(&ctr->walks_served, served);
      atomic_add_u64(&usage[0], served);
    }
    if (over) {
      atomic_add_u64(&ctr->walks_over, over);
      atomic_add_u64(&usage[1], over);
    }
  }
}

// one walk per thread, terminals written out (walker parity tests, pprhip_random_walk_batch)
__global__ __launch_bounds__(256) void k_walk_batch(const int32_t* __restrict__ starts,
                                                     const unsigned long long* __restrict__ idx,
                                                     unsigned long long count,
                                                     const unsigned long long* __restrict__ out_ext,
                                                     const uint4* __restrict__ walk_rec,
                                                     const int32_t* __restrict__ new2old, double alpha, uint32_t k0,
                                                     uint32_t k1, uint32_t stream, int no_zero_hop,
                                                     int32_t* __restrict__ term, uint32_t* __restrict__ steps) {
  for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < count;
       i += (unsigned long long)gridDim.x * blockDim.x) {
    const int32_t s = starts[i];
    Walker w;
    const unsigned long long sext = out_ext[s];
    walker_init(w, s, sext, new2old[s], idx[i], stream, no_zero_hop != 0);
    if ((sext >> 32) != 0) {
      while (!walker_step(w, walk_rec, alpha, k0, k1)) {
      }
    }
    term[i] = w.cur;
    if (steps) steps[i] = w.moves;
  }
}

// edge records of the walk kernel, built once at graph lift
__global__ __launch_bounds__(256) void k_build_walk_rec(unsigned long long m, const int32_t* __restrict__ out_ci,
                                                         const unsigned long long* __restrict__ out_ext,
                                                         uint4* __restrict__ walk_rec) {
  for (unsigned long long e = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; e < m;
       e += (unsigned long long)gridDim.x * blockDim.x) {
    const int32_t u = out_ci[e];
    const unsigned long long ext = out_ext[u];
    walk_rec[e] = make_uint4((uint32_t)u, (uint32_t)ext, (uint32_t)(ext >> 32), 0u);
  }
}

__global__ void k_plan_single(int32_t src, double inc, unsigned long long n_walks,
                              const unsigned long long* __restrict__ out_ext, const int32_t* __restrict__ new2old,
                              WalkPlanRec* plan, DevCounters* ctr, int parity, int next_cell) {
  WalkPlanRec r;
  r.woff = 0ull;
  r.inc = inc;
  r.ext = out_ext[src];
  r.node = src;
  r.orig = new2old[src];
  plan[0] = r;
  ctr->mc_plan[next_cell] = 0ull;
  ctr->mc_plan[parity] = (1ull << kPackShift) | n_walks;
}

// ------------------------------------------------------------------------------------------------
// single pairs (pprhip_ppr_pairs, DESIGN.md §2 "Single pairs")
// ------------------------------------------------------------------------------------------------
// One Jacobi iteration of the leaking walk's survival over the out-CSR: S'(u) = alpha + (1 - alpha) / d(u) *
// sum_{u->v} S(v), alpha at dead ends.  A row of out-degree < kSurvHeavy is summed by a group of kSurvLanes lanes
// (k_survival_iter); the few longer ones (the hubs of an R-MAT graph: a thread-per-row form of the kernel, whose waves wait
// for their longest row, took 10.3 s for the whole solve at R-MAT 22) by a whole workgroup each (k_survival_heavy).  check != 0: max |S' - S|
// goes to *dmax (non-negative doubles order as their bit patterns, so an integer maximum serves).
constexpr uint32_t kSurvLanes = 8;
constexpr uint32_t kSurvHeavy = 512;

__device__ __forceinline__ void surv_max_out(unsigned long long mx, unsigned long long* __restrict__ dmax) {
  __shared__ unsigned long long s_max[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_down(mx, o);
    mx = y > mx ? y : mx;
  }
  if (lane_id() == 0) s_max[wave_id()] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) mx = s_max[w] > mx ? s_max[w] : mx;
    if (mx) atomicMax(dmax, mx);
  }
}

__device__ __forceinline__ unsigned long long surv_diff_bits(double x, double old) {
  const double dx = fabs(x - old);
  unsigned long long bits;
  __builtin_memcpy(&bits, &dx, 8);
  return bits;
}

__global__ __launch_bounds__(256) void k_survival_iter(uint32_t n, const unsigned long long* __restrict__ out_ext,
                                                        const int32_t* __restrict__ out_ci, const double* __restrict__ s_old,
                                                        double* __restrict__ s_new, double alpha, int check,
                                                        unsigned long long* __restrict__ dmax) {
  unsigned long long mx = 0ull;
  const uint32_t sub = threadIdx.x % kSurvLanes;
  const uint32_t groups = gridDim.x * (256u / kSurvLanes);
  for (uint32_t u = (blockIdx.x * 256u + threadIdx.x) / kSurvLanes; u < n; u += groups) {  // (uniform per group)
    const unsigned long long ext = out_ext[u];
    const uint32_t b = (uint32_t)ext, d = (uint32_t)(ext >> 32);
    if (d >= kSurvHeavy) continue;
    double sum = 0.0;
    for (uint32_t j = sub; j < d; j += kSurvLanes) sum += s_old[out_ci[b + j]];
#pragma unroll
    for (uint32_t o = kSurvLanes / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (sub == 0) {
      const double x = d ? alpha + (1.0 - alpha) * sum / (double)d : alpha;
      s_new[u] = x;
      if (check) {
        const unsigned long long bits = surv_diff_bits(x, s_old[u]);
        mx = bits > mx ? bits : mx;
      }
    }
  }
  if (check) surv_max_out(mx, dmax);
}

__global__ __launch_bounds__(256) void k_survival_heavy(const int32_t* __restrict__ rows, uint32_t count,
                                                         const unsigned long long* __restrict__ out_ext,
                                                         const int32_t* __restrict__ out_ci,
                                                         const double* __restrict__ s_old, double* __restrict__ s_new,
                                                         double alpha, int check, unsigned long long* __restrict__ dmax) {
  __shared__ double s_red[4];
  unsigned long long mx = 0ull;
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const int32_t u = rows[i];
    const unsigned long long ext = out_ext[u];
    const uint32_t b = (uint32_t)ext, d = (uint32_t)(ext >> 32);
    double sum = 0.0;
    for (uint32_t j = threadIdx.x; j < d; j += 256u) sum += s_old[out_ci[b + j]];
    sum = block_sum_f64(sum, s_red);
    if (threadIdx.x == 0) {
      const double x = alpha + (1.0 - alpha) * sum / (double)d;
      s_new[u] = x;
      if (check) {
        const unsigned long long bits = surv_diff_bits(x, s_old[u]);
        mx = bits > mx ? bits : mx;
      }
    }
  }
  if (check) surv_max_out(mx, dmax);
}

// Gather walks of one target's sources: work item (p, c) = the walks [c * chunk_walks, min(w, (c + 1) * chunk_walks))
// of pair p, one wave per item.  The walks are pprhip_random_walk_batch's (walker_init / walker_step, stream
// PPRHIP_PAIR_WALK_STREAM, no zero-hop skip); a lane whose walk has stopped adds residue[terminal] to its register and
// takes the item's next walk (refill in ballot order, so which lane runs which walk depends on the item alone).  The
// wave's sum goes to part[p * chunks + c]: no atomics on a pair's value, the same bits in every call.
__global__ __launch_bounds__(64) void k_pair_walk(const int32_t* __restrict__ src, uint32_t n_pairs, uint32_t chunks,
                                                   unsigned long long chunk_walks, unsigned long long walks,
                                                   const unsigned long long* __restrict__ out_ext,
                                                   const uint4* __restrict__ walk_rec, const int32_t* __restrict__ new2old,
                                                   const double* __restrict__ residue, double alpha, uint32_t k0,
                                                   uint32_t k1, double* __restrict__ part,
                                                   unsigned long long* __restrict__ steps_out) {
  const int lane = threadIdx.x;
  const unsigned long long items = (unsigned long long)n_pairs * chunks;
  unsigned long long steps = 0;
  for (unsigned long long it = blockIdx.x; it < items; it += gridDim.x) {
    const uint32_t p = (uint32_t)(it / chunks), c = (uint32_t)(it % chunks);
    const int32_t s = src[p];
    const unsigned long long sext = out_ext[s];
    const int32_t s_orig = new2old[s];
    const unsigned long long lo = (unsigned long long)c * chunk_walks;
    const unsigned long long hi = lo + chunk_walks < walks ? lo + chunk_walks : walks;
    unsigned long long cursor = lo;
    double acc = 0.0;
    Walker w;
    bool walking = false;
    for (;;) {
      const unsigned long long need = __ballot(!walking);
      if (need && cursor < hi) {
        const unsigned long long avail = hi - cursor;
        const uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
        if (!walking && rank < avail) {
          walker_init(w, s, sext, s_orig, cursor + rank, PPRHIP_PAIR_WALK_STREAM, false);
          if ((sext >> 32) == 0) acc += residue[s];  // a dead-end start is its own terminal (k_walk_batch)
          else walking = true;
        }
        const unsigned long long want = __popcll(need);
        cursor += want < avail ? want : avail;
      }
      if (__ballot(walking) == 0) {
        if (cursor >= hi) break;
        continue;
      }
      if (walking && walker_step(w, walk_rec, alpha, k0, k1)) {
        acc += residue[w.cur];
        steps += w.moves;
        walking = false;
      }
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) part[(size_t)p * chunks + c] = acc;
  }
  steps = wave_sum_u64(steps);
  if (lane == 0 && steps) atomic_add_u64(steps_out, steps);
}

// value of pair p = p_t(s) / S(s) + (sum of its chunks, in chunk order) / w, written at the pair's place in the call
__global__ __launch_bounds__(256) void k_pair_reduce(const int32_t* __restrict__ src, const int32_t* __restrict__ pos,
                                                      uint32_t n_pairs, uint32_t chunks, const double* __restrict__ part,
                                                      double walks, const double* __restrict__ reserve,
                                                      const double* __restrict__ survival, double* __restrict__ values) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_pairs) return;
  const int32_t s = src[p];
  double sum = 0.0;
  for (uint32_t c = 0; c < chunks; ++c) sum += part[(size_t)p * chunks + c];
  double v = reserve[s] / survival[s];
  if (chunks) v += sum / walks;
  values[pos[p]] = v;
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
int launch_survival_iter(pprhip_graph* g, const double* s_old, double* s_new, double alpha, const int32_t* d_heavy,
                         uint32_t n_heavy, unsigned long long* dmax) {
  const uint32_t n = g->gr->n;
  const uint64_t b = ((uint64_t)n * kSurvLanes + 255) / 256;
  const uint32_t grid = (uint32_t)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
  hipLaunchKernelGGL(k_survival_iter, dim3(grid), dim3(256), 0, g->stream, n, g->gr->out_ext, g->gr->out_ci, s_old, s_new,
                     alpha, dmax ? 1 : 0, dmax);
  PPRHIP_CHECK_HIP(hipGetLastError());
  if (n_heavy) {
    hipLaunchKernelGGL(k_survival_heavy, dim3(std::min<uint32_t>(n_heavy, 4096u)), dim3(256), 0, g->stream, d_heavy,
                       n_heavy, g->gr->out_ext, g->gr->out_ci, s_old, s_new, alpha, dmax ? 1 : 0, dmax);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  return PPRHIP_OK;
}

uint32_t survival_heavy_degree() { return kSurvHeavy; }

int launch_pair_walk(pprhip_graph* g, const int32_t* d_src, uint32_t n_pairs, uint32_t chunks, uint64_t chunk_walks,
                     uint64_t walks, double alpha, uint64_t seed, double* d_part, unsigned long long* d_steps) {
  const uint64_t items = (uint64_t)n_pairs * chunks;
  if (items == 0) return PPRHIP_OK;
  const uint64_t cap = (uint64_t)g->gr->n_cus * kWalkWavesPerCu;
  const uint32_t grid = (uint32_t)(items < cap ? items : cap);
  hipLaunchKernelGGL(k_pair_walk, dim3(grid), dim3(64), 0, g->stream, d_src, n_pairs, chunks,
                     (unsigned long long)chunk_walks, (unsigned long long)walks, g->gr->out_ext,
                     reinterpret_cast<const uint4*>(g->gr->walk_rec), g->gr->new2old, g->residue, alpha, (uint32_t)seed,
                     (uint32_t)(seed >> 32), d_part, d_steps);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_pair_reduce(pprhip_graph* g, const int32_t* d_src, const int32_t* d_pos, uint32_t n_pairs, uint32_t chunks,
                       const double* d_part, uint64_t walks, const double* survival, double* d_values) {
  if (n_pairs == 0) return PPRHIP_OK;
  hipLaunchKernelGGL(k_pair_reduce, dim3((n_pairs + 255) / 256), dim3(256), 0, g->stream, d_src, d_pos, n_pairs, chunks,
                     d_part, (double)walks, g->reserve, survival, d_values);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int init_kernels_walk() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_mc_walk<kWalkPlain>)));
  return PPRHIP_OK;
}

int launch_build_walk_rec(pprhip_graph* g) {
  if (g->gr->m == 0) return PPRHIP_OK;
  hipLaunchKernelGGL(k_build_walk_rec, dim3(4096), dim3(256), 0, g->stream, (unsigned long long)g->gr->m, g->gr->out_ci,
                     g->gr->out_ext, reinterpret_cast<uint4*>(g->gr->walk_rec));
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// the phase a plan belongs to picks its counter cell and its record buffer; the next walk kernel runs the latest plan
static WalkPlanRec* plan_rec_of(pprhip_graph* g, uint32_t phase) {
  return (g->mc_plan_rec2 && (phase & 1u)) ? g->mc_plan_rec2 : g->mc_plan_rec;
}

int launch_mc_plan(pprhip_graph* g, int variant, double alpha, double rsum, double nrw, double omega_dev, double* target,
                   const double* copy_src, double* copy_dst) {
  const uint32_t phase = g->mc_phase++;
  g->mc_last_plan = phase;
  const int cell = (int)(phase % 3u), next_cell = (int)((phase + 1u) % 3u);
  const uint32_t n = act_n(g);
  uint64_t b = ((uint64_t)n + 1023) / 1024;  // 1024 nodes per workgroup (fewer or more were slower)
  const uint64_t cap = g->sync ? 1024 : 16384;  // (a slot of a threaded batch: see launch_seed_list)
  const uint32_t grid = (uint32_t)(b > cap ? cap : (b < 1 ? 1 : b));
  const uint32_t np = g->sum_np;  // partial sums a launch_sum_partial has just left for this plan (0: none)
  g->sum_np = 0;
  if (variant == 1 && omega_dev > 0.0 && np > 0) {
    const uint32_t tiles = (n + 256u * kPlanItems - 1) / (256u * kPlanItems);
    hipLaunchKernelGGL(k_mc_plan_topk, dim3(std::max(1u, tiles)), dim3(256), 0, g->stream, n, g->residue, alpha, omega_dev,
                       g->partial, np, g->gr->out_ext, g->gr->new2old, plan_rec_of(g, phase), g->ctr, cell, next_cell, copy_src,
                       copy_dst);
  } else if (variant == 0)
    hipLaunchKernelGGL(k_mc_plan<0>, dim3(grid), dim3(256), 0, g->stream, n, g->residue, target, alpha, rsum, nrw,
                       omega_dev, g->gr->out_ext, g->gr->new2old, plan_rec_of(g, phase), g->ctr, cell, next_cell, copy_src, copy_dst);
  else
    hipLaunchKernelGGL(k_mc_plan<1>, dim3(grid), dim3(256), 0, g->stream, n, g->residue, target, alpha, rsum, nrw,
                       omega_dev, g->gr->out_ext, g->gr->new2old, plan_rec_of(g, phase), g->ctr, cell, next_cell, copy_src, copy_dst);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// The walk count is only known on the device: a fixed grid of waves, each with an equal share of whatever the plan
// holds (g->walk_hint, the budget when the host knows it, only trims the grid of a short phase).
static uint32_t mc_walk_grid(pprhip_graph* g) {
  // (walk_waves: a walk phase that runs beside other kernels leaves them room - the walks are bound by the memory
  // system from a few waves per CU on, tools/micro/chain_rate.hip)
  // a slot of a threaded batch shares the chip with fifteen others: few waves per CU, like a walk phase beside sweeps
  // (batched top-k on R-MAT 22: 851 queries/s at 16 waves per CU, 961 / 1 026 / 905 at 2 / 4 / 8)
  uint32_t grid = (uint32_t)g->gr->n_cus * (g->walk_waves ? g->walk_waves
                                        : g->sync   ? kWalkWavesBeside
                                                    : kWalkWavesPerCu);
  if (g->walk_hint) grid = (uint32_t)std::min<unsigned long long>(grid, std::max<unsigned long long>((g->walk_hint + 63) / 64, 1ull));
  g->walk_hint = 0;
  return grid;
}

int launch_mc_walk(pprhip_graph* g, double alpha, uint64_t seed, uint32_t stream, int no_zero_hop, double* target) {
  const uint32_t grid = mc_walk_grid(g);
  hipLaunchKernelGGL(k_mc_walk<kWalkPlain>, dim3(grid), dim3(64), 0, g->stream, plan_rec_of(g, g->mc_last_plan),
                     reinterpret_cast<const uint4*>(g->gr->walk_rec), target, alpha, (uint32_t)seed, (uint32_t)(seed >> 32), stream,
                     no_zero_hop, g->ctr, (int)(g->mc_last_plan % 3u), (const unsigned long long*)nullptr,
                     (uint32_t*)nullptr, 0u, (unsigned long long*)nullptr, (int)kDepAtomic, (uint32_t*)nullptr,
                     (double*)nullptr, 0ull, 0ull);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// The same grid for both kernels: the serve kernel's share of a wave is a stream of terminals, the walk kernel behind
// it returns at once unless the serve kernel counted walks the index does not hold.
int launch_index_serve(pprhip_graph* g, const TerminalTable* ix, double* target, uint32_t grid) {
  hipLaunchKernelGGL(k_index_serve, dim3(grid), dim3(64), 0, g->stream, plan_rec_of(g, g->mc_last_plan), ix->off, ix->term,
                     target, g->ctr, (int)(g->mc_last_plan % 3u), ix->usage);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_mc_walk_indexed(pprhip_graph* g, const TerminalTable* ix, double alpha, uint64_t seed, double* target) {
  const uint32_t grid = mc_walk_grid(g);
  const int cell = (int)(g->mc_last_plan % 3u);
  PPRHIP_TRY(launch_index_serve(g, ix, target, grid));
  hipLaunchKernelGGL(k_mc_walk<kWalkIndexed>, dim3(grid), dim3(64), 0, g->stream, plan_rec_of(g, g->mc_last_plan),
                     reinterpret_cast<const uint4*>(g->gr->walk_rec), target, alpha, (uint32_t)seed, (uint32_t)(seed >> 32), 0u,
                     1, g->ctr, cell, (const unsigned long long*)ix->off, (uint32_t*)nullptr, 0u,
                     (unsigned long long*)nullptr, (int)kDepAtomic, (uint32_t*)nullptr, (double*)nullptr, 0ull, 0ull);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_mc_walk_shared(pprhip_graph* g, const TerminalTable* ws, double alpha, uint64_t seed, double* target,
                          const WalkDeposit* dep) {
  const uint32_t grid = mc_walk_grid(g);
  // measurement switch, read per call: PPRHIP_WALK_DEPOSIT=none runs the phase without its deposits
  const char* sw = hook_env("PPRHIP_WALK_DEPOSIT");
  const int dep_mode = sw && sw[0] == 'n' ? kDepNone : dep && dep->on ? kDepBinned : kDepAtomic;
  DepositArgs a;
  if (dep_mode == kDepBinned) a = dep->a;
  // measurement switch, read per call: PPRHIP_WALK_DEPOSIT_SKIP=count|scatter|sum, the pass that stores nothing
  const char* skip = hook_env("PPRHIP_WALK_DEPOSIT_SKIP");
  a.skip = !skip ? kDepSkipNone : skip[0] == 'c' ? kDepSkipCount : skip[0] == 's' && skip[1] == 'c' ? kDepSkipScatter
         : skip[0] == 's' && skip[1] == 'u' ? kDepSkipSum : kDepSkipNone;
  const int cell = (int)(g->mc_last_plan % 3u);
  hipLaunchKernelGGL(k_mc_walk<kWalkShared>, dim3(grid), dim3(64), 0, g->stream, plan_rec_of(g, g->mc_last_plan),
                     reinterpret_cast<const uint4*>(g->gr->walk_rec), target, alpha, (uint32_t)seed, (uint32_t)(seed >> 32), 0u,
                     1, g->ctr, cell, (const unsigned long long*)ws->off, (uint32_t*)ws->term, g->gr->n, ws->usage, dep_mode,
                     a.key, a.inc, (unsigned long long)a.cap, (unsigned long long)a.min_walks);
  PPRHIP_CHECK_HIP(hipGetLastError());
  if (dep_mode == kDepBinned) {
    // one workgroup per CU: the sweeps on the other stream keep theirs (kernels_dense_batch.hip)
    const uint32_t wg = (uint32_t)g->gr->n_cus;
    hipLaunchKernelGGL(k_dep_count, dim3(wg), dim3(256), 0, g->stream, a, (const DevCounters*)g->ctr, cell);
    hipLaunchKernelGGL(k_dep_items, dim3(1), dim3(256), 0, g->stream, a, (const DevCounters*)g->ctr, cell);
    hipLaunchKernelGGL(k_dep_bin, dim3(wg), dim3(256), 0, g->stream, a, (const DevCounters*)g->ctr, cell);
    hipLaunchKernelGGL(k_dep_tile, dim3(wg), dim3(256), 0, g->stream, a, (const DevCounters*)g->ctr, cell);
    hipLaunchKernelGGL(k_dep_sum, dim3(wg), dim3(256), 0, g->stream, a, (const DevCounters*)g->ctr, cell, target);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  return PPRHIP_OK;
}

int launch_index_build(pprhip_graph* g, const TerminalTable* ix, unsigned long long* d_steps) {
  if (ix->total == 0) return PPRHIP_OK;
  const uint64_t cap = (uint64_t)g->gr->n_cus * kWalkWavesPerCu;
  const uint64_t groups = (ix->total + 63) / 64;
  const uint32_t grid = (uint32_t)(groups < cap ? groups : cap);
  hipLaunchKernelGGL(k_index_build, dim3(grid), dim3(64), 0, g->stream, ix->off, g->gr->n, (unsigned long long)ix->total,
                     g->gr->out_ext, reinterpret_cast<const uint4*>(g->gr->walk_rec), g->gr->new2old, ix->alpha,
                     (uint32_t)ix->seed, (uint32_t)(ix->seed >> 32), ix->term, d_steps);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_walk_batch(pprhip_graph* g, const int32_t* d_starts, const uint64_t* d_idx, uint64_t count, double alpha,
                      uint64_t seed, uint32_t stream, int no_zero_hop, int32_t* d_term, uint32_t* d_steps) {
  if (count == 0) return PPRHIP_OK;
  uint64_t b = (count + 255) / 256;
  const uint32_t grid = (uint32_t)(b > 4096 ? 4096 : b);
  hipLaunchKernelGGL(k_walk_batch, dim3(grid), dim3(256), 0, g->stream, d_starts,
                     (const unsigned long long*)d_idx, (unsigned long long)count, g->gr->out_ext, g->gr->walk_rec, g->gr->new2old, alpha,
                     (uint32_t)seed, (uint32_t)(seed >> 32), stream, no_zero_hop, d_term, d_steps);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_mc_pure(pprhip_graph* g, int32_t src, uint64_t n_walks, double alpha, uint64_t seed, double inc,
                   double* target) {
  const uint32_t phase = g->mc_phase++;
  g->mc_last_plan = phase;
  hipLaunchKernelGGL(k_plan_single, dim3(1), dim3(1), 0, g->stream, src, inc, (unsigned long long)n_walks, g->gr->out_ext,
                     g->gr->new2old, plan_rec_of(g, phase), g->ctr, (int)(phase % 3u), (int)((phase + 1u) % 3u));
  PPRHIP_CHECK_HIP(hipGetLastError());
  return launch_mc_walk(g, alpha, seed, 0, 0, target);
}

}  // namespace pprhip
