// kernels_weighted_topk_batch.hip — the merged walk launch of the batched weighted top-k calls for gfx950 (MI355X;
// DESIGN.md §2 "Batched weighted top-k"; weighted_topk_batch.cpp drives it).  A weighted top-k round's walk phase is
// small - 0.4 - 8 M walks over a query's rounds - and lasts as long as its longest walk, so sixteen of them one after
// another leave most of the chip idle.  k_w_walk_plan_multi runs the walk plans of every column that is ready in one
// launch: the waves are dealt to the columns by their walk counts (walk_multi_deal, weighted_batch.hpp - the counts are
// known on the device only, so every wave reads the sixteen plan cells and derives the same shares), no wave spans two
// columns, and inside its share a wave runs k_w_walk_plan<false>'s loop as it stands: refill in ballot order, the
// entry by binary search from the wave's oldest open walk, a dead-end start its own terminal, one fp64 atomic per walk
// at the terminal.  Walk (seed_c, stream_c, node, index) of column c is the walk its single call runs.  (The dead-end
// start branch is never taken for the plan of a top-k round - no round ends with residue on a dead end - and no test
// runs it; it stays because the loop is k_w_walk_plan's.)
#include "weighted_batch.hpp"
#include "weighted_device.hpp"

namespace pprhip {

struct WalkMultiTable {
  WalkMultiCol col[kBatch];
};

// One workgroup = one wave.  Everything chosen per column is wave-uniform and lives in SGPRs: the table is read with
// constant indices only (no scratch).
__global__ __launch_bounds__(64) void k_w_walk_plan_multi(WWalkGraph G, double alpha, WalkMultiTable tab,
                                                           uint32_t base_waves) {
  unsigned long long counts[kBatch];
#pragma unroll
  for (int c = 0; c < kBatch; ++c) {
    const DevCounters* ctr = tab.col[c].ctr;
    counts[c] = ctr ? (ctr->mc_plan[tab.col[c].cell] & kPackMask) : 0ull;
  }
  unsigned long long per = 0;
  uint32_t first[kBatch + 1];
  walk_multi_deal(counts, base_waves, &per, first);
  const uint32_t b = blockIdx.x;
  // the column this wave works for, and - waves 0 .. 15 - the column whose totals it adds (also a plan of sources
  // without walks is counted)
  WalkMultiCol mine{}, tot{};
  unsigned long long n_walks = 0, lo_wave = 0;
  bool have = false;
#pragma unroll
  for (int c = 0; c < kBatch; ++c) {
    if (b >= first[c] && b < first[c + 1]) {
      mine = tab.col[c];
      n_walks = counts[c];
      lo_wave = first[c];
      have = true;
    }
    if (b == (uint32_t)c) tot = tab.col[c];
  }
  if (tot.ctr && threadIdx.x == 0) {
    const unsigned long long plan = tot.ctr->mc_plan[tot.cell];
    tot.ctr->walks_total += plan & kPackMask;
    tot.ctr->sources_total += plan >> kPackShift;
  }
  if (!have) return;
  const WalkPlanRec* __restrict__ plan_rec = mine.plan_rec;
  double* __restrict__ target = mine.target;
  DevCounters* const ctr = mine.ctr;
  const uint32_t n_src = (uint32_t)(ctr->mc_plan[mine.cell] >> kPackShift);
  const uint32_t k0 = mine.k0, k1 = mine.k1, stream = mine.stream;
  const int lane = threadIdx.x;
  unsigned long long cursor = ((unsigned long long)b - lo_wave) * per;
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
        uint32_t a = e_lo + 1u, z = n_src;
        while (a < z) {
          const uint32_t mid = (a + z) >> 1;
          if (plan_rec[mid].woff <= gidx) a = mid + 1u; else z = mid;
        }
        e = a - 1u;
        const WalkPlanRec r = plan_rec[e];
        inc = r.inc;
        w_walker_init(w, r.node, r.ext, r.orig, gidx - r.woff, stream, false);
        if ((r.ext >> 32) == 0)
          atomic_add_noret(&target[r.node], inc);  // a dead-end start is its own terminal
        else
          walking = true;
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

// ------------------------------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------------------------------
// The latest walk plans of the workspaces cols[c] (nullptr: column c is idle) in one launch on the parent's stream:
// column c's walks are (seeds[c], streams[c], node, index) without the forced first hop, added into its estimate
// targets[c].  The base grid is launch_w_walk_run's, trimmed by the sum of the columns' walk hints when every column
// has one; the hints are consumed.  (The only caller's plans carry none: a top-k plan derives its budget on the device
// and launch_walk_plan leaves walk_hint = 0, so the base is always n_cus * 16 there; the trim is launch_w_walk_run's rule,
// kept for a caller whose host knows a bound.)
int launch_w_walk_multi(pprhip_graph* P, pprhip_graph* const* cols, const uint64_t* seeds, const uint32_t* streams,
                        double* const* targets, double alpha) {
  const GraphData* D = P->gr;
  WalkMultiTable tab;
  unsigned long long hint = 0;
  bool hinted = true;
  int busy = 0;
  for (int c = 0; c < kBatch; ++c) {
    WalkMultiCol& m = tab.col[c];
    m = WalkMultiCol{};
    pprhip_graph* S = cols[c];
    if (!S) continue;
    m.plan_rec = (S->mc_plan_rec2 && (S->mc_last_plan & 1u)) ? S->mc_plan_rec2 : S->mc_plan_rec;
    m.target = targets[c];
    m.ctr = S->ctr;
    m.cell = (int)(S->mc_last_plan % 3u);
    m.k0 = (uint32_t)seeds[c];
    m.k1 = (uint32_t)(seeds[c] >> 32);
    m.stream = streams[c];
    hinted = hinted && S->walk_hint != 0;
    hint += S->walk_hint;
    S->walk_hint = 0;
    busy++;
  }
  if (!busy) return PPRHIP_OK;
  uint32_t base = (uint32_t)D->n_cus * 16u;
  if (hinted) base = (uint32_t)std::min<unsigned long long>(base, std::max<unsigned long long>((hint + 63) / 64, 1ull));
  // walk_multi_deal uses at most base + kBatch - 1 waves, and at least kBatch are there for the columns' totals
  const uint32_t grid = base + (uint32_t)kBatch - 1u;
  k_w_walk_plan_multi<<<dim3(grid), dim3(64), 0, P->stream>>>(
      WWalkGraph{D->out_ext, D->out_ci, D->out_cum, D->wsum}, alpha, tab, base);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int init_kernels_weighted_topk_batch() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_w_walk_plan_multi)));
  return PPRHIP_OK;
}

}  // namespace pprhip
