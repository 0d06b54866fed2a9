// run.hpp — one query as a resumable run (ForaRun) and the five kinds of run: whole-graph FORA, FORA top-k, a backward
// search of All-Pair, the push and walks of a pair call, the push and scaling of a single-target query.  fora.cpp
// defines the first two, bwd_runs.cpp the three that push backward; the batch drivers (batch.cpp) and the query stream
// (stream.cpp) step them.
#pragma once

#include <algorithm>
#include <cmath>

#include "engine_internal.hpp"

namespace pprhip {

// Fora_Topk.java's schedule on delta: the push's floor (:113), a round's thresholds (:124-125) and the push's
// threshold (:133), the end of the loop (:175-176) and the next delta (:178)
struct TopkSchedule {
  double eps = 0, min_delta = 0, m = 0, lg = 0, min_rmax = 0;
  TopkSchedule() = default;
  TopkSchedule(double eps_half, const pprhip_fora_conf_t* conf)
      : eps(eps_half), min_delta(conf->min_delta), m((double)conf->m), lg(std::log(2.0 / conf->pfail)),
        min_rmax(rmax(min_delta)) {}
  double rmax(double delta) const { return eps * std::sqrt(delta / 3.0 / m / lg); }
  double omega(double delta) const { return (eps + 2.0) * lg / eps / eps / delta; }
  double push_rmax(double rmax) const { return rmax * (std::sqrt(m * rmax) * 3.0); }
  bool last(double kth, double delta) const { return kth >= (1 + eps) * delta || delta <= min_delta; }
  double next(double delta) const { return std::max(min_delta, delta / 4.0); }
};

// One FORA query as a resumable run: step() advances it until it is finished or (yield_dense)
// until its next level is dense, so that the batch driver can run that level for many queries
// in one sweep.  pprhip_fora_single_source drives the same code without yielding.
struct ForaRun {
  pprhip_graph* g = nullptr;
  int32_t src = 0;  // internal id
  const pprhip_fora_conf_t* conf = nullptr;
  uint64_t seed = 0;
  int n_rounds = 0;
  detail::CallTimer* tm = nullptr;  // single-query calls: push / walk phase marks
  pprhip_stats_t st;
  double alpha = 0, rsum_local = 0, rmax_local = 0, omega_local = 0, rmax_used = 0, model_cost = 0;
  int rounds = 0;
  bool dead_src = false;
  bool seeded = false;  // a seed set (g->seeds) instead of src: src = -1 in the push arguments
  detail::LevelCtx L;
  PushArgs a;
  detail::RoundCut cut;
  enum Phase { kRoundStart, kLevels, kWalks, kWalkWait, kTopkRoundStart, kTopkLevels, kTopkRoundEnd, kTopkFinal, kBwdLevels,
               kBwdFinal, kDone } phase = kDone;  // kBwdLevels / kBwdFinal: every run that pushes backward (bwd_runs.cpp)
  hipStream_t side = nullptr;  // batch driver: the walk phase goes to this stream and the run yields until it has ended
  int query = -1;  // batch driver: index of the query this run serves
  detail::BatchJob* job = nullptr;  // ... and the call (or stream submission) that query belongs to
  bool waiting = false;
  bool in_push = false;  // between a push phase's start and its end (BatchSync: may hold sweeps off)
  // top-k runs (Fora_Topk.computeTopKPPR, kTopk): the trial-and-error loop on delta
  detail::QueryKind kind = detail::QueryKind::kFora;
  TopkSchedule sched;
  double delta_local = 0, kth_prev = -1.0;  // (kth_prev: the k-th estimate of the round before; -1: none yet)
  uint32_t round = 0;
  int cap = 0, nsel = 0;
  int32_t* ids_out = nullptr;
  double* vals_out = nullptr;
  // ... options of the single-query driver (pprhip_fora_topk): the next round's push runs ahead on the handle's second
  // stream (ahead), the walks run at walk_waves waves per CU (0: the handle's width), each phase is marked by an event
  // and timed (marks: push_ms / mc_ms / sel_ms)
  bool ahead = false, marks = false;
  uint32_t walk_waves = 0;
  double push_ms = 0, mc_ms = 0, sel_ms = 0;
  bool pushed_ahead = false;     // this round's push, residue sum and walk plan have already run (second stream)
  bool ahead_pending = false;    // a push ahead is queued and the compute stream has not joined it yet
  bool ahead_discarded = false;  // the last push ahead was not needed
  unsigned long long dead_before_ahead = 0;
  // the runs that push backward (kBwdLevels, then kBwdFinal finishes by kind)
  bool lone = false;  // the single target src has no in-edges: no level ran, src is the only entry of the vector
  // backward searches of All-Pair (kBackward): entries >= threshold of the finished search
  int32_t target_orig = -1;
  std::vector<detail::Triple> triples;
  // single pairs (kPairs): after the push the walks of the sorted pairs [pair_lo, pair_hi) - none for a lone target
  const detail::PairPlan* pp = nullptr;
  uint32_t pair_lo = 0, pair_hi = 0;
  // single targets (kTargets): after the push the division by S and the delivery of the vector
  const detail::TargetPlan* tp = nullptr;
  double push_t0 = 0.0;  // host clock at the query's begin (ms): push_ms is wall time on the workspace
};

}  // namespace pprhip

namespace pprhip {
namespace detail {

// *_begin starts a query on the workspace g (its vectors are reset); *_step advances it until it has finished
// (PPRHIP_OK, phase kDone) or yields (kYield*, engine_internal.hpp; only with yield_dense, or a run with a side stream)
int fora_begin(ForaRun& r, pprhip_graph* g, int32_t src_internal, double eps, const pprhip_fora_conf_t* conf,
               uint64_t seed, int n_rounds);
int fora_begin_seeds(ForaRun& r, pprhip_graph* g, SeedTable& plan, double eps, const pprhip_fora_conf_t* conf,
                     uint64_t seed, int n_rounds);
int fora_step(ForaRun& r, bool yield_dense);
int topk_begin(ForaRun& r, pprhip_graph* g, int32_t src_internal, double eps, const pprhip_fora_conf_t* conf,
               uint64_t seed, int32_t* ids_out, double* vals_out, int cap);
int topk_begin_seeds(ForaRun& r, pprhip_graph* g, SeedTable& plan, double eps, const pprhip_fora_conf_t* conf,
                     uint64_t seed, int32_t* ids_out, double* vals_out, int cap);
int topk_step(ForaRun& r, bool yield_dense);
int bwd_begin(ForaRun& r, pprhip_graph* g, int32_t target_internal, int32_t target_orig, double alpha, double rmax);
int pair_begin(ForaRun& r, pprhip_graph* g, const PairPlan& pp, int32_t target_internal, uint32_t lo, uint32_t hi);
int target_begin(ForaRun& r, pprhip_graph* g, const TargetPlan& tp, int i);  // set i of the plan
int bwd_step(ForaRun& r, bool yield_dense);  // the step of all three
int run_step(ForaRun& r, bool yield_dense);  // the step of r's kind
void leave_push(ForaRun& r);                 // the run's push phase is over (or given up): it stops holding sweeps off
// omega and the threshold a whole-graph FORA query's first push runs at (every later one runs at a lower one)
int fora_start_params(const pprhip_graph* g, double eps, const pprhip_fora_conf_t* conf, int n_rounds, double* rmax_out,
                      double* omega_out);
void add_stats(pprhip_stats_t& sum, const pprhip_stats_t& st);
void add_push_stats(pprhip_stats_t& sum, const pprhip_stats_t& st);  // the counters of a push that ran ahead

}  // namespace detail
}  // namespace pprhip
