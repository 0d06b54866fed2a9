// forward_calls.cpp — the front end of the forward single-query calls, weighted and unweighted: the four forward push
// calls, the two weighted whole-graph FORA calls and the two walk-batch calls.  Every entry point is a wrapper of its
// own checks, in its documented order, around one body per family.  A body is told where the push starts (one source
// or a seed plan) and whether it runs over w / W (run_weighted_levels, weighted.cpp) or over 1 / d (run_levels,
// levels.cpp); nothing else differs between the calls.  The unweighted FORA and top-k runs are in fora.cpp, the
// weighted top-k loop in weighted_query.cpp.
#include <cstring>
#include <vector>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace {

// Where a forward push starts: one source (internal id, checked), which pops unconditionally first, or a seed plan
// (seeds.cpp), whose table receives the dead-end mass of every level (SeedScope).  The two stay apart: a single
// source is not the set {s}.
struct Start {
  int32_t src = -1;
  SeedTable* plan = nullptr;
};

// the first frontier on a workspace just reset; L.nf stays 0 when there is nothing to push: a dead-end source leaves
// reserve = e_s (Forward_Push.java:72-76), a set without a live seed reserve = p
template <class Levels>
int first_frontier(pprhip_graph* g, const Start& s, Levels& L) {
  if (s.plan) return seed_start(g, L);
  const uint32_t d = hdeg_out(g, s.src);
  if (d == 0) return launch_set_f64(g, g->reserve, (uint32_t)s.src, 1.0);
  PPRHIP_TRY(launch_set_f64(g, g->residue, (uint32_t)s.src, 1.0));
  PPRHIP_TRY(launch_seed_one(g, L.fcur, s.src));  // (Forward_Push.java:81-86)
  L.nf = 1;
  L.ef = d;
  return PPRHIP_OK;
}

// the workspace reset for a query from s, the plan installed
int begin_query(pprhip_graph* g, const Start& s) {
  g->topk_active = false;
  PPRHIP_TRY(reset_query_state(g, false, s.plan ? s.plan->max_id : s.src));
  return s.plan ? seed_upload(g, *s.plan) : PPRHIP_OK;
}

// One push from s at rmax, run to its end.  *live: something was pushed; *sum: the residue sum (0 when nothing was).
int push_to_end(pprhip_graph* g, const Start& s, bool weighted, double alpha, double rmax, pprhip_stats_t& st, double* sum,
                bool* live) {
  *sum = 0.0;
  SeedScope scope(g, s.plan != nullptr);
  const PushArgs a{alpha, rmax, 0.0, s.plan ? -1 : s.src, kFwdWhole};
  if (weighted) {
    WLevels L;
    PPRHIP_TRY(first_frontier(g, s, L));
    *live = L.nf != 0;
    if (*live) PPRHIP_TRY(run_weighted_levels(g, a, L, st));
  } else {
    LevelCtx L;
    PPRHIP_TRY(first_frontier(g, s, L));
    *live = L.nf != 0;
    if (*live) PPRHIP_TRY(run_levels(g, a, L, st, nullptr));
  }
  return *live ? device_sum(g, g->residue, sum) : PPRHIP_OK;
}

// The four forward push calls behind their checks.
int forward_push(pprhip_graph* g, const Start& s, bool weighted, double alpha, double rmax, double* reserve_out,
                 double* residue_out, double* rsum_out, pprhip_stats_t* stats) {
  pprhip_stats_t st;
  std::memset(&st, 0, sizeof st);
  PPRHIP_TRY(begin_query(g, s));
  CallTimer tm(g);
  double rsum = 0.0;
  bool live = false;
  PPRHIP_TRY(push_to_end(g, s, weighted, alpha, rmax, st, &rsum, &live));
  if (live) PPRHIP_TRY(read_dead_pops(g, st));  // (nothing pushed: every counter it reads was just reset to zero)
  tm.mark(1);
  tm.finish(st);
  st.push_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  st.rsum = rsum;
  st.rmax_final = rmax;
  st.rounds = 1;
  if (rsum_out) *rsum_out = rsum;
  PPRHIP_TRY(copy_out(g, g->reserve, reserve_out));
  PPRHIP_TRY(copy_out(g, g->residue, residue_out));
  if (stats) *stats = st;
  return PPRHIP_OK;
}

// Both weighted whole-graph FORA calls behind their checks: one push at rmax (0: rmax0), then the walk plan of the
// unweighted whole-graph FORA, unchanged (k_mc_plan<0>), with weighted walks - where something was pushed.
int weighted_fora(pprhip_graph* g, const Start& s, double eps, const pprhip_fora_conf_t* conf, uint64_t seed, double rmax,
                  double* reserve_out, pprhip_stats_t* stats) {
  double rmax0 = 0.0, omega = 0.0;
  PPRHIP_TRY(pprhip_fora_whole_params(conf, eps, &rmax0, &omega));
  if (rmax == 0.0) rmax = rmax0;
  const double alpha = conf->alpha;
  pprhip_stats_t st;
  std::memset(&st, 0, sizeof st);
  PPRHIP_TRY(begin_query(g, s));
  CallTimer tm(g);
  double sum = 0.0;
  bool live = false;
  PPRHIP_TRY(push_to_end(g, s, true, alpha, rmax, st, &sum, &live));
  tm.mark(1);
  const double rsum = sum * (1 - alpha);
  if (live) {
    const double nrw_d = omega * rsum;
    const long long nrw = (nrw_d == nrw_d && nrw_d > 0.0) ? (long long)nrw_d : 0;
    PPRHIP_TRY(launch_walk_plan(g, 0, alpha, rsum, nrw, g->reserve, 0.0));
    ktimer().begin(PPRHIP_KERNEL_WALK, 0);
    PPRHIP_TRY(launch_w_walk_run(g, alpha, seed, g->reserve, 0u, true));
    ktimer().end();
  }
  tm.mark(2);
  PPRHIP_TRY(read_dead_pops(g, st));
  st.rounds = 1;
  st.rsum = rsum;
  st.rmax_final = rmax;
  st.omega = omega;
  tm.finish(st);
  st.push_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  st.mc_ms = CallTimer::ms(g->ev[1], g->ev[2]);
  PPRHIP_TRY(copy_out(g, g->reserve, reserve_out));
  if (stats) *stats = st;
  return PPRHIP_OK;
}

// Both walk-batch calls behind alpha, the handle and (weighted) the weights: walk i is (seed, stream, starts[i],
// walk_idx[i]); the caller's ids in and out.
int walk_batch(pprhip_graph* g, bool weighted, const int32_t* starts, const uint64_t* walk_idx, uint64_t count,
               double alpha, uint64_t seed, uint32_t stream, int no_zero_hop, int32_t* terminals_out, uint32_t* steps_out,
               const char* fn) {
  if ((!starts || !walk_idx || !terminals_out) && count) {
    set_error("%s: null argument", fn);
    return PPRHIP_ERR_INVALID;
  }
  if (stream >= 65536) {
    set_error("%s: stream must be < 65536", fn);
    return PPRHIP_ERR_INVALID;
  }
  for (uint64_t i = 0; i < count; ++i)  // (check_node's test inline: millions of starts per call)
    if (!node_in_range(g, starts[i])) return check_node(g, starts[i], fn);
  if (count == 0) return PPRHIP_OK;
  int32_t *d_s = nullptr, *d_t = nullptr;
  uint64_t* d_i = nullptr;
  uint32_t* d_n = nullptr;
  auto done = [&](int code) {
    (void)hipFree(d_s); (void)hipFree(d_t); (void)hipFree(d_i); (void)hipFree(d_n);
    return code;
  };
  int rc = PPRHIP_OK;
  if ((rc = alloc_dev((void**)&d_s, sizeof(int32_t) * count)) || (rc = alloc_dev((void**)&d_t, sizeof(int32_t) * count)) ||
      (rc = alloc_dev((void**)&d_i, sizeof(uint64_t) * count)) || (rc = alloc_dev((void**)&d_n, sizeof(uint32_t) * count)))
    return done(rc);
  std::vector<int32_t> mapped(count);
  for (uint64_t i = 0; i < count; ++i) mapped[i] = g->gr->h_old2new[starts[i]];
  if (hipMemcpy(d_s, mapped.data(), sizeof(int32_t) * count, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpyAsync(d_i, walk_idx, sizeof(uint64_t) * count, hipMemcpyHostToDevice, g->stream) != hipSuccess) {
    set_error("%s: upload failed", fn);
    return done(PPRHIP_ERR_HIP);
  }
  rc = (weighted ? launch_w_walk_batch : launch_walk_batch)(g, d_s, d_i, count, alpha, seed, stream, no_zero_hop, d_t, d_n);
  if (rc) return done(rc);
  if (hipMemcpyAsync(terminals_out, d_t, sizeof(int32_t) * count, hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
      (steps_out &&
       hipMemcpyAsync(steps_out, d_n, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, g->stream) != hipSuccess) ||
      hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error("%s: download failed: %s", fn, hipGetErrorString(hipGetLastError()));
    return done(PPRHIP_ERR_HIP);
  }
  for (uint64_t i = 0; i < count; ++i) terminals_out[i] = g->gr->h_new2old[terminals_out[i]];
  return done(PPRHIP_OK);
}

}  // namespace

// The checks the weighted FORA calls (and their batched forms, weighted_batch.cpp) run before they look at the handle.
int pprhip::detail::check_weighted_fora_params(double eps, const pprhip_fora_conf_t* conf, double rmax, const char* fn) {
  PPRHIP_TRY(check_positive(eps, fn, "eps"));
  PPRHIP_TRY(check_conf(conf, fn, false));
  PPRHIP_TRY(check_threshold(rmax, fn, "rmax"));
  if (!conf) {
    set_error("%s: null conf", fn);
    return PPRHIP_ERR_INVALID;
  }
  return PPRHIP_OK;
}

extern "C" {

// ------------------------------------------------------------------ forward push (a1)
int pprhip_forward_push(pprhip_graph_t* g, int32_t src, double alpha, double rmax, double* reserve_out,
                        double* residue_out, double* rsum_out, pprhip_stats_t* stats) {
  static const char* fn = "pprhip_forward_push";
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_threshold(rmax, fn, "rmax"));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(check_node(g, src, fn));
  const Start s{g->gr->h_old2new[src], nullptr};
  return forward_push(g, s, false, alpha, rmax, reserve_out, residue_out, rsum_out, stats);
}

int pprhip_weighted_forward_push(pprhip_graph_t* g, int32_t src, double alpha, double rmax, double* reserve_out,
                                 double* residue_out, double* rsum_out, pprhip_stats_t* stats) {
  static const char* fn = "pprhip_weighted_forward_push";
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_threshold(rmax, fn, "rmax"));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  PPRHIP_TRY(check_node(g, src, fn));
  const Start s{g->gr->h_old2new[src], nullptr};
  return forward_push(g, s, true, alpha, rmax, reserve_out, residue_out, rsum_out, stats);
}

int pprhip_forward_push_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds,
                              double alpha, double rmax, double* reserve_out, double* residue_out, double* rsum_out,
                              pprhip_stats_t* stats) {
  static const char* fn = "pprhip_forward_push_seeds";
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_threshold(rmax, fn, "rmax"));
  PPRHIP_TRY(check_graph(g, fn));
  SeedTable plan;
  PPRHIP_TRY(seed_plan(g, seeds, weights, n_seeds, alpha, fn, plan));
  return forward_push(g, Start{-1, &plan}, false, alpha, rmax, reserve_out, residue_out, rsum_out, stats);
}

int pprhip_weighted_forward_push_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds,
                                       double alpha, double rmax, double* reserve_out, double* residue_out,
                                       double* rsum_out, pprhip_stats_t* stats) {
  static const char* fn = "pprhip_weighted_forward_push_seeds";
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_threshold(rmax, fn, "rmax"));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  SeedTable plan;
  PPRHIP_TRY(seed_plan(g, seeds, weights, n_seeds, alpha, fn, plan));
  return forward_push(g, Start{-1, &plan}, true, alpha, rmax, reserve_out, residue_out, rsum_out, stats);
}

// ------------------------------------------------------------------ weighted whole-graph FORA
int pprhip_weighted_fora(pprhip_graph_t* g, int32_t src, double eps, const pprhip_fora_conf_t* conf, uint64_t seed,
                         double rmax, double* reserve_out, pprhip_stats_t* stats) {
  static const char* fn = "pprhip_weighted_fora";
  PPRHIP_TRY(check_weighted_fora_params(eps, conf, rmax, fn));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  PPRHIP_TRY(check_node(g, src, fn));
  const Start s{g->gr->h_old2new[src], nullptr};
  return weighted_fora(g, s, eps, conf, seed, rmax, reserve_out, stats);
}

int pprhip_weighted_fora_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds, double eps,
                               const pprhip_fora_conf_t* conf, uint64_t seed, double rmax, double* reserve_out,
                               pprhip_stats_t* stats) {
  static const char* fn = "pprhip_weighted_fora_seeds";
  PPRHIP_TRY(check_weighted_fora_params(eps, conf, rmax, fn));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  SeedTable plan;
  PPRHIP_TRY(seed_plan(g, seeds, weights, n_seeds, conf->alpha, fn, plan));
  return weighted_fora(g, Start{-1, &plan}, eps, conf, seed, rmax, reserve_out, stats);
}

// ------------------------------------------------------------------ walker exposure (a3, a4)
int pprhip_random_walk_batch(pprhip_graph_t* g, const int32_t* starts, const uint64_t* walk_idx, uint64_t count,
                             double alpha, uint64_t seed, uint32_t stream, int no_zero_hop, int32_t* terminals_out,
                             uint32_t* steps_out) {
  static const char* fn = "pprhip_random_walk_batch";
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_graph(g, fn));
  return walk_batch(g, false, starts, walk_idx, count, alpha, seed, stream, no_zero_hop, terminals_out, steps_out, fn);
}

int pprhip_weighted_random_walk_batch(pprhip_graph_t* g, const int32_t* starts, const uint64_t* walk_idx, uint64_t count,
                                      double alpha, uint64_t seed, uint32_t stream, int no_zero_hop, int32_t* terminals_out,
                                      uint32_t* steps_out) {
  static const char* fn = "pprhip_weighted_random_walk_batch";
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  return walk_batch(g, true, starts, walk_idx, count, alpha, seed, stream, no_zero_hop, terminals_out, steps_out, fn);
}

}  // extern "C"
