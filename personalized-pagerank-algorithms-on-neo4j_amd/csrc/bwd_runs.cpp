// bwd_runs.cpp — the three kinds of run that push backward (run.hpp): a backward search of All-Pair, the push and walks
// of a pair call, the push and scaling of a single-target query.  They share the start of the push (backward_start,
// which pprhip_backward_push uses too), its levels (bwd_step) and differ in what follows the push: the finishers below.
// The walk blocks of a pair target (pair_walk_blocks) serve the weighted pair call (weighted_bwd.cpp) as well.
#include <algorithm>
#include <cstring>

#include "run.hpp"

namespace pprhip {
namespace detail {

int backward_start(pprhip_graph* g, LevelCtx& L, PushArgs& a, int32_t target_internal, double alpha, double rmax,
                   double lone_value, bool* pushing) {
  *pushing = hdeg_in(g, target_internal) > 0;
  if (!*pushing) return launch_set_f64(g, g->reserve, (uint32_t)target_internal, lone_value);
  a = PushArgs{alpha, rmax, 0.0, target_internal, kBackward};
  L = LevelCtx();
  PPRHIP_TRY(launch_set_f64(g, g->residue, (uint32_t)target_internal, 1.0));
  return seed_single(g, L, target_internal, hdeg_in(g, target_internal));
}

// what every backward run's begin sets before it resets the workspace
static void bwd_prologue(ForaRun& r, pprhip_graph* g, QueryKind kind, int32_t src, double alpha, double rmax) {
  r.g = g;
  r.kind = kind;
  r.src = src;
  r.alpha = alpha;
  r.rmax_local = rmax;
  std::memset(&r.st, 0, sizeof r.st);
  g->topk_active = false;
  r.waiting = false;
  r.in_push = false;
}

// the push from the single target r.src on the workspace that has just been reset
static int bwd_start_single(ForaRun& r, double lone_value) {
  bool pushing = false;
  PPRHIP_TRY(backward_start(r.g, r.L, r.a, r.src, r.alpha, r.rmax_local, lone_value, &pushing));
  r.lone = !pushing;
  r.in_push = pushing;
  r.phase = pushing ? ForaRun::kBwdLevels : ForaRun::kBwdFinal;
  return PPRHIP_OK;
}

// One backward search of All-Pair (Backward_Search.java:38-100 + the >= threshold filter of
// Base_Whole_Graph.java:80-88) as a resumable run.
int bwd_begin(ForaRun& r, pprhip_graph* g, int32_t target_internal, int32_t target_orig, double alpha, double rmax) {
  bwd_prologue(r, g, QueryKind::kBackward, target_internal, alpha, rmax);
  r.target_orig = target_orig;
  r.triples.clear();
  PPRHIP_TRY(reset_query_state(g, false, target_internal));
  return bwd_start_single(r, 1.0);
}

// The backward push of a pair call (BatchJob kPairs), then the walks of the sorted pairs [lo, hi).
int pair_begin(ForaRun& r, pprhip_graph* g, const PairPlan& pp, int32_t target_internal, uint32_t lo, uint32_t hi) {
  bwd_prologue(r, g, QueryKind::kPairs, target_internal, pp.alpha, pp.rmax);
  r.pp = &pp;
  r.pair_lo = lo;
  r.pair_hi = hi;
  if (g->ws_index < 0 || g->ws_index >= kBatch) {
    set_error("pair call: workspace %d has no pair buffers", g->ws_index);
    return PPRHIP_ERR_STATE;
  }
  PPRHIP_TRY(reset_query_state(g, false, target_internal));
  PPRHIP_CHECK_HIP(hipEventRecord(pp.ev[3 * g->ws_index], g->stream));
  return bwd_start_single(r, pp.alpha);
}

// A single-target query (BatchJob kTargets, targets.cpp): the backward push from set i of the call's table at the
// call's threshold, under the handle's tuning, then value = p / S in place of the reserve (k_target_finish), which the
// batch driver delivers like a whole-graph vector (top-k, result store, values_out).  A single target starts as a
// pair's target does; a set starts from r = w (k_target_init), its first frontier known to the host.
int target_begin(ForaRun& r, pprhip_graph* g, const TargetPlan& tp, int i) {
  bwd_prologue(r, g, QueryKind::kTargets, tp.single[(size_t)i], tp.alpha, tp.rmax);
  r.tp = &tp;
  PPRHIP_TRY(reset_query_state(g, false, tp.max_id[(size_t)i]));
  r.push_t0 = host_ms();
  if (r.src >= 0) return bwd_start_single(r, tp.alpha);
  r.a = PushArgs{tp.alpha, tp.rmax, 0.0, -1, kBackward};
  r.L = LevelCtx();
  // (the list counter is zero: reset_query_state cleared the counters, and a level's first prepare clears it again)
  {
    SetupScope setup(g);
    PPRHIP_TRY(launch_target_init(g, tp.d_id + tp.first[(size_t)i], tp.d_w + tp.first[(size_t)i], tp.count[(size_t)i],
                                  r.L.fcur, &g->ctr->hist[kMaxBatch + 2], tp.alpha, tp.rmax));
  }
  r.L.nf = tp.nf[(size_t)i];
  r.L.ef = tp.ef[(size_t)i];
  r.L.dense_prepared = false;
  r.L.gs_dirty = false;
  r.lone = false;
  r.in_push = true;
  r.phase = ForaRun::kBwdLevels;
  return PPRHIP_OK;
}

// kBackward: the entries >= threshold of the finished search as triples (Base_Whole_Graph.java:83 pi >= threshold)
static int finish_search(ForaRun& r) {
  pprhip_graph* g = r.g;
  const double threshold = r.rmax_local;
  unsigned long long thr_bits = 1ull;
  if (threshold > 0.0) std::memcpy(&thr_bits, &threshold, 8);
  PPRHIP_TRY(launch_select_gather(g, g->reserve, act_n(g), thr_bits, true));
  unsigned long long cnt = 0;
  PPRHIP_TRY(fetch_small(g, g->sel_blob, &cnt, sizeof cnt));
  const std::vector<int32_t>& n2o = g->gr->h_new2old;
  if (cnt > g->sel_cap) {
    std::vector<double> all(g->gr->n);
    PPRHIP_TRY(copy_out(g, g->reserve, all.data()));
    for (uint32_t v = 0; v < g->gr->n; ++v)  // copy_out already returned original ids
      if (all[v] > 0.0 && all[v] >= threshold) r.triples.push_back({(int32_t)v, r.target_orig, all[v]});
  } else if (cnt) {
    std::vector<SelRec> recs(cnt);
    PPRHIP_CHECK_HIP(hipMemcpyAsync(recs.data(), g->sel_blob + kSelHeader, sizeof(SelRec) * cnt, hipMemcpyDeviceToHost, g->stream));
    PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    for (uint64_t i = 0; i < cnt; ++i) r.triples.push_back({n2o[recs[i].id], r.target_orig, recs[i].val});
  }
  return PPRHIP_OK;
}

int pair_walk_blocks(pprhip_graph* g, const PairPlan& pp, uint32_t lo, uint32_t hi, double* part, bool lone,
                     decltype(&launch_pair_walk) walk, pprhip_stats_t& st) {
  const uint32_t chunks = lone ? 0u : pp.chunks;
  ktimer().begin(PPRHIP_KERNEL_WALK, 0);
  for (uint32_t b = lo; b < hi; b += pp.block_pairs) {
    const uint32_t np = std::min(pp.block_pairs, hi - b);
    if (chunks) PPRHIP_TRY(walk(g, pp.d_src + b, np, chunks, pp.chunk_walks, pp.walks, pp.alpha, pp.seed, part, pp.d_steps));
    PPRHIP_TRY(launch_pair_reduce(g, pp.d_src + b, pp.d_pos + b, np, chunks, part, pp.walks, pp.survival, pp.d_values));
  }
  ktimer().end();
  if (chunks) {
    st.walks += pp.walks * (uint64_t)(hi - lo);
    st.mc_sources += hi - lo;
  }
  return PPRHIP_OK;
}

// kPairs: the walks of the target's sources and their values, between the workspace's second and third event
static int finish_pairs(ForaRun& r) {
  pprhip_graph* g = r.g;
  const PairPlan& pp = *r.pp;
  const int ws = g->ws_index;
  PPRHIP_CHECK_HIP(hipEventRecord(pp.ev[3 * ws + 1], g->stream));
  PPRHIP_TRY(pair_walk_blocks(g, pp, r.pair_lo, r.pair_hi, pp.d_part + (size_t)ws * pp.part_cap, r.lone, launch_pair_walk,
                              r.st));
  PPRHIP_CHECK_HIP(hipEventRecord(pp.ev[3 * ws + 2], g->stream));
  r.st.rounds = 1;
  return PPRHIP_OK;
}

// kTargets: value = p / S in place of the reserve
static int finish_targets(ForaRun& r) {
  pprhip_graph* g = r.g;
  r.st.push_ms = host_ms() - r.push_t0;  // (the last level's counters have been read: the push is over on the device)
  {
    SetupScope setup(g);
    PPRHIP_TRY(launch_target_finish(g, r.tp->survival, act_n(g), r.lone ? r.src : -1));
  }
  r.st.rmax_final = r.rmax_local;
  r.st.rounds = 1;
  return PPRHIP_OK;
}

int bwd_step(ForaRun& r, bool yield_dense) {
  if (r.phase == ForaRun::kBwdLevels) {
    const int rc = run_levels(r.g, r.a, r.L, r.st, nullptr, yield_dense);
    if (rc != PPRHIP_OK) return rc;  // kYield or an error
    leave_push(r);
    r.phase = ForaRun::kBwdFinal;
  }
  if (r.phase == ForaRun::kBwdFinal) {  // the push is over (or there was none): finish by kind
    switch (r.kind) {
      case QueryKind::kBackward: PPRHIP_TRY(finish_search(r)); break;
      case QueryKind::kPairs: PPRHIP_TRY(finish_pairs(r)); break;
      case QueryKind::kTargets: PPRHIP_TRY(finish_targets(r)); break;
      case QueryKind::kFora:
      case QueryKind::kTopk:
        set_error("bwd_step: not a backward run");
        return PPRHIP_ERR_STATE;
    }
    r.phase = ForaRun::kDone;
  }
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip
