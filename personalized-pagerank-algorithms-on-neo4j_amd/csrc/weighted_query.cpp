// weighted_query.cpp — weighted FORA top-k (include/pprhip.h "weighted seed sets and top-k"):
// pprhip_weighted_fora_topk and pprhip_weighted_fora_topk_seeds.  Both run one loop: a weighted push that starts from
// a seed table (here a single source is the set {s} with weight 1), lands dead-end mass on p, and is resumed at a
// lower threshold round after round.  The driver is a small loop of its own over run_weighted_levels (weighted.cpp):
// plain rounds, no parking or arming, no push ahead, no cost model.  The seed table, the walk plan, the selection and
// the getters are the unweighted engine's.  The weighted seed-set push and FORA calls are in forward_calls.cpp.
#include <cstring>

#include "weighted_batch.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace {

// levels at rmax from L's frontier to their end, dead-end mass landing on the seed table
int seeded_levels(pprhip_graph* g, double alpha, double rmax, WLevels& L, pprhip_stats_t& st) {
  SeedScope scope(g);
  const PushArgs a{alpha, rmax, 0.0, -1, kFwdWhole};
  return run_weighted_levels(g, a, L, st);
}

// The checks of both entry points up to the start, in their order.  src: the caller's single source, checked between
// the weights and the output row (NULL: a seed set, which the caller parses after them).
int topk_checks(pprhip_graph* g, const int32_t* src, double eps, const pprhip_fora_conf_t* conf, int cap,
                const int32_t* ids_out, const double* vals_out, const char* fn) {
  PPRHIP_TRY(check_positive(eps, fn, "eps"));
  PPRHIP_TRY(check_conf(conf, fn, true));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  if (src) PPRHIP_TRY(check_node(g, *src, fn));
  return topk_args_ok(conf, eps, cap, ids_out, vals_out, fn) ? PPRHIP_OK : PPRHIP_ERR_INVALID;
}

}  // namespace

// The weighted top-k loop on delta (Fora_Topk.java's schedule: nothing in it depends on the weights) from the seed
// table `plan`.
int pprhip::detail::weighted_topk_drive(pprhip_graph* g, SeedTable& plan, double eps, const pprhip_fora_conf_t* conf,
                                        uint64_t seed, int32_t* ids_out, double* vals_out, int cap, int* n_out,
                                        double* reserve_out, pprhip_stats_t* stats) {
  const double alpha = conf->alpha;
  const TopkSchedule sc(eps * 0.5, conf);
  pprhip_stats_t st;
  std::memset(&st, 0, sizeof st);
  g->topk_active = false;
  PPRHIP_TRY(reset_query_state(g, false, plan.max_id));
  PPRHIP_TRY(seed_upload(g, plan));
  WLevels L0;
  PPRHIP_TRY(seed_start(g, L0));
  const size_t nd = sizeof(double) * (size_t)act_n(g);  // (est beyond the query's scan bound is zero and stays so)
  CallTimer tm(g);
  double push_ms = 0.0, mc_ms = 0.0, sel_ms = 0.0;
  double delta = conf->delta, rmax_j = 0.0, omega_j = 0.0, rsum = conf->rsum, kth = 0.0;
  uint32_t round = 0;
  int nsel = 0;
  bool have = false;
  if (g->seeds->n_live == 0) {  // the estimate is p: rounds = 0, one selection
    PPRHIP_CHECK_HIP(hipMemcpyAsync(g->est, g->reserve, nd, hipMemcpyDeviceToDevice, g->stream));
    rsum = 0.0;
    tm.mark(3);
    PPRHIP_TRY(select_topk(g, g->est, conf->k, ids_out, vals_out, cap, &nsel, &kth, &have, st));
    tm.mark(4);
    PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    sel_ms += CallTimer::ms(g->ev[3], g->ev[4]);
  } else {
    unsigned long long* const cell = &g->ctr->hist[0];
    for (;;) {
      rmax_j = sc.push_rmax(sc.rmax(delta));
      omega_j = sc.omega(delta);
      tm.mark(1);
      WLevels L = L0;  // round 0: the live seeds
      if (round > 0) {  // every node active at the new threshold (possibly none: straight to the walks)
        L = WLevels();
        PPRHIP_CHECK_HIP(hipMemsetAsync(cell, 0, sizeof(unsigned long long), g->stream));
        {
          SetupScope setup(g);
          PPRHIP_TRY(launch_wq_collect(g, rmax_j, L.fcur, cell));
        }
        PPRHIP_TRY(fetch_packed(g, cell, &L.nf, &L.ef));
        st.enqueues += L.nf;
      }
      PPRHIP_TRY(seeded_levels(g, alpha, rmax_j, L, st));
      // est := reserve, then the plan of the unweighted top-k rounds, its budget derived on the device
      PPRHIP_TRY(launch_sum_partial(g, g->residue, act_n(g)));
      PPRHIP_TRY(launch_walk_plan(g, 1, alpha, 0.0, 0, g->est, omega_j, g->reserve, g->est));
      tm.mark(2);
      ktimer().begin(PPRHIP_KERNEL_WALK, 0);  // (its bytes are added when the counters are read)
      PPRHIP_TRY(launch_w_walk_run(g, alpha, seed, g->est, round, false));
      ktimer().end();
      tm.mark(3);
      round++;
      PPRHIP_TRY(select_topk(g, g->est, conf->k, ids_out, vals_out, cap, &nsel, &kth, &have, st, true));
      rsum = g->sel_plan_sum;  // (the residue sum this round's plan was derived from, as the unweighted rounds report it)
      if (!have) kth = 0.0;
      tm.mark(4);
      PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
      push_ms += CallTimer::ms(g->ev[1], g->ev[2]);
      mc_ms += CallTimer::ms(g->ev[2], g->ev[3]);
      sel_ms += CallTimer::ms(g->ev[3], g->ev[4]);
      if (sc.last(kth, delta)) break;
      delta = sc.next(delta);
    }
  }
  g->result_in_est = true;
  PPRHIP_TRY(read_dead_pops(g, st));
  tm.finish(st);
  st.push_ms = push_ms;
  st.mc_ms = mc_ms;
  st.select_ms = sel_ms;
  st.rounds = round;
  st.kth_value = kth;
  st.rsum = rsum;
  st.rmax_final = rmax_j;
  st.omega = omega_j;
  if (n_out) *n_out = nsel;
  for (int i = std::max(nsel, 0); i < cap; ++i) {  // the row's unused entries
    ids_out[i] = -1;
    vals_out[i] = 0.0;
  }
  PPRHIP_TRY(copy_out(g, g->est, reserve_out));
  if (stats) *stats = st;
  return PPRHIP_OK;
}

extern "C" {

int pprhip_weighted_fora_topk(pprhip_graph_t* g, int32_t src, double eps, const pprhip_fora_conf_t* conf, uint64_t seed,
                              int32_t* ids_out, double* vals_out, int cap, int* n_out, double* reserve_out,
                              pprhip_stats_t* stats) {
  static const char* fn = "pprhip_weighted_fora_topk";
  PPRHIP_TRY(topk_checks(g, &src, eps, conf, cap, ids_out, vals_out, fn));
  SeedTable plan;
  PPRHIP_TRY(seed_plan(g, &src, nullptr, 1, conf->alpha, fn, plan));  // the set {src} with weight 1
  return weighted_topk_drive(g, plan, eps, conf, seed, ids_out, vals_out, cap, n_out, reserve_out, stats);
}

int pprhip_weighted_fora_topk_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds,
                                    double eps, const pprhip_fora_conf_t* conf, uint64_t seed, int32_t* ids_out,
                                    double* vals_out, int cap, int* n_out, double* reserve_out, pprhip_stats_t* stats) {
  static const char* fn = "pprhip_weighted_fora_topk_seeds";
  PPRHIP_TRY(topk_checks(g, nullptr, eps, conf, cap, ids_out, vals_out, fn));
  SeedTable plan;
  PPRHIP_TRY(seed_plan(g, seeds, weights, n_seeds, conf->alpha, fn, plan));
  return weighted_topk_drive(g, plan, eps, conf, seed, ids_out, vals_out, cap, n_out, reserve_out, stats);
}

}  // extern "C"
