// weighted_bwd.cpp — the backward direction over weighted relationships (include/pprhip.h "weighted relationships",
// DESIGN.md §2 "Weighted backward direction"): the weighted backward push, the weighted survival vector S_w, single
// targets / target sets and single pairs over P(u, v) = w / W(u), as a small driver over kernels_weighted_bwd.hip.
// A target call of two or more queries runs batched, its dense levels on a shared 16-column sweep
// (weighted_bwd_batch.cpp); a call of one, the pairs' targets and All-Pair's whole-vector searches run one after another
// on the handle's own workspace.  What is specific to the weights is here - which kernels run and the serial loops.
// Everything else is shared with the unweighted calls: the level loop (weighted.cpp: run_weighted_levels), the front of
// a target call (targets.cpp: target_plan), the front and back of a pair call and the survival iteration (pairs.cpp:
// pair_plan / pair_upload / pair_collect, survival_jacobi), a pair target's walk blocks (bwd_runs.cpp:
// pair_walk_blocks), and around a query the workspace and its reset, the start of a target set and the division by S
// (kernels_target.hip), the pair reduction (kernels_walk.hip), the delivery helpers, the getters.
#include <algorithm>
#include <cstring>

#include "run.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace {

// The push from one target (internal id) on a workspace just reset: r(t) = 1 and t pops unconditionally first.  A
// target without in-edges gets reserve(t) = lone_value and no push (*lone): 1.0 for pprhip_weighted_backward_push,
// alpha for targets and pairs (bwd_runs.cpp: backward_start).
int weighted_bwd_single(pprhip_graph* g, int32_t t, double alpha, double rmax, double lone_value, pprhip_stats_t& st,
                        bool* lone) {
  *lone = hdeg_in(g, t) == 0;
  if (*lone) return launch_set_f64(g, g->reserve, (uint32_t)t, lone_value);
  const PushArgs a{alpha, rmax, 0.0, t, kBackward};
  WLevels L;
  PPRHIP_TRY(launch_set_f64(g, g->residue, (uint32_t)t, 1.0));
  PPRHIP_TRY(launch_seed_one(g, L.fcur, t));
  L.nf = 1;
  L.ef = hdeg_in(g, t);
  return run_weighted_levels(g, a, L, st);
}

// S_w at alpha on the lifted graph (pairs.cpp: survival_jacobi; both buffers start from S0: the rows without out-edges
// keep alpha in either).  Kept per alpha beside the unweighted S; goes with the weights (free_weights).
int ensure_weighted_survival(pprhip_graph* g, double alpha) {
  GraphData* D = g->gr;
  if (D->wsurvival && D->wsurvival_alpha == alpha) return PPRHIP_OK;
  PPRHIP_TRY(ensure_bwd_layout(g));
  if (D->wsurvival) (void)hipFree(D->wsurvival);
  D->wsurvival = nullptr;
  PPRHIP_TRY(survival_jacobi(g, alpha, "pprhip_weighted_walk_survival", true, D->m == 0,
                             [&](const double* s_old, double* s_new, unsigned long long* dmax) {
                               return launch_wb_survival_iter(g, s_old, s_new, alpha, dmax);
                             },
                             &D->wsurvival));
  D->wsurvival_alpha = alpha;
  return PPRHIP_OK;
}

}  // namespace

// (All-Pair's whole-vector searches over the weights, allpair.cpp)
int pprhip::detail::weighted_backward_search_whole(pprhip_graph_t* g, int32_t target, double alpha, double rmax,
                                                   pprhip_stats_t& st) {
  PPRHIP_TRY(reset_query_state(g, false, target));
  bool lone = false;
  return weighted_bwd_single(g, target, alpha, rmax, 1.0, st, &lone);
}

extern "C" {

int pprhip_weighted_backward_push(pprhip_graph_t* g, int32_t target, double alpha, double rmax, double* reserve_out,
                                  double* residue_out, pprhip_stats_t* stats) {
  static const char* fn = "pprhip_weighted_backward_push";
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_threshold(rmax, fn, "rmax"));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  PPRHIP_TRY(check_node(g, target, fn));
  target = g->gr->h_old2new[target];  // internal id
  pprhip_stats_t st;
  std::memset(&st, 0, sizeof st);
  g->topk_active = false;
  CallTimer tm(g);
  PPRHIP_TRY(reset_query_state(g, false, target));
  bool lone = false;
  PPRHIP_TRY(weighted_bwd_single(g, target, alpha, rmax, 1.0, st, &lone));
  tm.mark(1);
  tm.finish(st);
  st.push_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  st.rmax_final = rmax;
  st.rounds = 1;
  PPRHIP_TRY(copy_out(g, g->reserve, reserve_out));
  PPRHIP_TRY(copy_out(g, g->residue, residue_out));
  if (stats) *stats = st;
  return PPRHIP_OK;
}

int pprhip_weighted_walk_survival(pprhip_graph_t* g, double alpha, double* survival_out) {
  static const char* fn = "pprhip_weighted_walk_survival";
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  PPRHIP_TRY(ensure_weighted_survival(g, alpha));
  return copy_out(g, g->gr->wsurvival, survival_out);
}

int pprhip_weighted_ppr_targets(pprhip_graph_t* g, const int32_t* targets, const double* weights, const uint64_t* offsets,
                                int q, double alpha, double rmax, pprhip_results_t* keep, double* values_out, int k,
                                int32_t* ids_out, double* vals_out, int* n_out, pprhip_stats_t* per_query,
                                pprhip_stats_t* stats_sum) {
  static const char* fn = "pprhip_weighted_ppr_targets";
  TargetPlan tp;
  PPRHIP_TRY(target_plan(g, targets, weights, offsets, q, alpha, rmax, keep, k, ids_out, vals_out, stats_sum, fn, true, tp));
  if (q == 0) return PPRHIP_OK;
  PPRHIP_TRY(ensure_weighted_survival(g, alpha));
  if (q >= 2) {  // up to kBatch queries in flight on the batch workspaces, their dense levels on one shared sweep
    tp.survival = g->gr->wsurvival;
    return weighted_targets_batch(g, tp, q, keep, values_out, k, ids_out, vals_out, n_out, per_query, stats_sum);
  }
  pprhip_stats_t sum;
  std::memset(&sum, 0, sizeof sum);
  g->topk_active = false;
  if (keep) keep->count = 0;
  const size_t n = g->gr->n;
  for (int i = 0; i < q; ++i) {  // the call of one, on the handle's own workspace
    const int32_t single = tp.single[(size_t)i];
    pprhip_stats_t st;
    std::memset(&st, 0, sizeof st);
    CallTimer tm(g);
    PPRHIP_TRY(reset_query_state(g, false, tp.max_id[(size_t)i]));
    const double t0 = host_ms();
    bool lone = false;
    if (single >= 0) {
      PPRHIP_TRY(weighted_bwd_single(g, single, alpha, rmax, alpha, st, &lone));
    } else {
      const PushArgs a{alpha, rmax, 0.0, -1, kBackward};
      WLevels L;
      // (the counter is zero: reset_query_state cleared the counters)
      PPRHIP_TRY(launch_target_init(g, tp.d_id + tp.first[(size_t)i], tp.d_w + tp.first[(size_t)i], tp.count[(size_t)i],
                                    L.fcur, &g->ctr->hist[kMaxBatch + 2], alpha, rmax));
      L.nf = tp.nf[(size_t)i];
      L.ef = tp.ef[(size_t)i];
      PPRHIP_TRY(run_weighted_levels(g, a, L, st));
    }
    st.push_ms = host_ms() - t0;
    // value = p / S_w in place of the reserve
    PPRHIP_TRY(launch_target_finish(g, g->gr->wsurvival, act_n(g), lone ? single : -1));
    // delivery (batch.cpp: deliver_vector)
    if (keep) PPRHIP_TRY(launch_copy_f64(g, g->reserve, keep->buf + (size_t)i * n, n));
    if (values_out) PPRHIP_TRY(copy_out(g, g->reserve, values_out + (size_t)i * n));
    if (k > 0) {
      int nsel = 0;
      bool have = false;
      int32_t* ids = ids_out + (size_t)i * k;
      double* vals = vals_out + (size_t)i * k;
      PPRHIP_TRY(select_topk(g, g->reserve, k, ids, vals, k, &nsel, nullptr, &have, st));
      for (int j = std::min(nsel, k); j < k; ++j) {
        ids[j] = -1;
        vals[j] = 0.0;
      }
      if (n_out) n_out[i] = nsel;
    }
    tm.finish(st);
    st.rmax_final = rmax;
    st.rounds = 1;
    if (per_query) per_query[i] = st;
    add_stats(sum, st);
  }
  if (hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error("%s: stream sync failed", fn);
    return PPRHIP_ERR_HIP;
  }
  if (keep) keep->count = q;
  if (stats_sum) {
    sum.rmax_final = rmax;
    *stats_sum = sum;
  }
  return PPRHIP_OK;
}

int pprhip_weighted_ppr_pairs(pprhip_graph_t* g, const int32_t* sources, const int32_t* targets, int q, double eps,
                              const pprhip_fora_conf_t* conf, double rmax, uint64_t seed, double* values_out,
                              pprhip_stats_t* stats_sum) {
  static const char* fn = "pprhip_weighted_ppr_pairs";
  PairPlan pp;
  PPRHIP_TRY(pair_plan(g, sources, targets, q, eps, conf, rmax, seed, values_out, stats_sum, fn, true, pp));
  if (q == 0) return PPRHIP_OK;
  PPRHIP_TRY(ensure_weighted_survival(g, pp.alpha));
  pp.survival = g->gr->wsurvival;
  PPRHIP_TRY(pair_upload(g, pp, 1, 0, fn));  // one workspace, timed by the handle's own events
  pprhip_stats_t sum;
  std::memset(&sum, 0, sizeof sum);
  g->topk_active = false;
  for (size_t i = 0; i < pp.distinct.size(); ++i) {  // one target at a time on the handle's own workspace
    const int32_t t = g->gr->h_old2new[pp.distinct[i]];
    pprhip_stats_t st;
    std::memset(&st, 0, sizeof st);
    CallTimer tm(g);
    PPRHIP_TRY(reset_query_state(g, false, t));
    tm.mark(1);
    bool lone = false;
    PPRHIP_TRY(weighted_bwd_single(g, t, pp.alpha, pp.rmax, pp.alpha, st, &lone));
    tm.mark(2);
    PPRHIP_TRY(pair_walk_blocks(g, pp, pp.first[i], pp.first[i + 1], pp.d_part, lone, launch_wb_pair_walk, st));
    tm.mark(3);
    tm.finish(st);
    st.push_ms = CallTimer::ms(g->ev[1], g->ev[2]);
    st.mc_ms = CallTimer::ms(g->ev[2], g->ev[3]);
    add_stats(sum, st);
  }
  return pair_collect(g, pp, values_out, sum, stats_sum, fn);
}

}  // extern "C"
