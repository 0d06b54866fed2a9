// weighted_topk_batch.cpp — batched weighted FORA top-k (include/pprhip.h "batched weighted top-k"):
// pprhip_weighted_fora_batch_topk and pprhip_weighted_fora_batch_topk_seeds.  Up to kBatch weighted top-k queries are
// in flight on the handle's batch workspaces.  The driver is weighted_batch.cpp's lockstep loop with a small state per
// column - levels, then walks, then the selection, then the next round or the delivery:
//   1. every column whose frontier is not empty runs one level - a sparse one on its own workspace, the dense ones in
//      one shared sweep (wbat_sparse_level / wbat_sweep, each column at its own round's threshold);
//   2. every column whose frontier has emptied plans its round's walks on its workspace, ONE launch walks the plans of
//      all of them (kernels_weighted_topk_batch.hip), and each selects on its workspace;
//   3. the selections are read, the host takes each column's decision - deliver, or the next delta and the collect of
//      the next round's first frontier - and one read-back brings the level counters and the collect counters;
//   4. a delivered column takes the call's next query.
// Query i takes, level by level and round by round, the decisions of pprhip_weighted_fora_topk(srcs[i], seed + i) /
// _seeds(set i, seed + i) (weighted_query.cpp: weighted_topk_drive); batching changes the order of additions only.  A
// column at a dense level never waits for another: the sweep runs with the columns that are dense this round (the plain
// rule of weighted_batch.cpp).  A call of one query runs weighted_topk_drive on the handle's own workspace.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "weighted_batch.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace {

struct WtbColumn {  // the top-k loop of the query on column c (WbatCall::q[c] holds its levels)
  enum Step { kLevels, kCollect } step = kLevels;  // kCollect: the round's first frontier is being counted
  double delta = 0.0, rmax_j = 0.0, omega_j = 0.0, kth = 0.0, rsum = 0.0;
  uint32_t round = 0;
  int nsel = 0;
  double t_mark = 0.0, push_ms = 0.0, mc_ms = 0.0, sel_ms = 0.0;  // host clock
  unsigned long long sel_seq = 0;
};

struct WtbCall {
  TopkSchedule sc;
  int k = 0;
  WtbColumn col[kBatch];
};

int32_t* row_ids(const BatchJob& J, int i) { return J.ids_out + (size_t)i * J.k; }
double* row_vals(const BatchJob& J, int i) { return J.vals_out + (size_t)i * J.k; }

// the thresholds of the column's round at its delta, and an empty level state (weighted_topk_drive's round start)
void wtb_round_params(WtbCall& T, WbatCall& C, int c) {
  WtbColumn& K = T.col[c];
  K.rmax_j = T.sc.push_rmax(T.sc.rmax(K.delta));
  K.omega_j = T.sc.omega(K.delta);
  C.q[c].a = PushArgs{C.alpha, K.rmax_j, 0.0, -1, kFwdWhole};
}

// The column's query is over: the statistics as weighted_topk_drive fills them, the delivery, the column free.
int wtb_deliver(WtbCall& T, WbatCall& C, int c) {
  pprhip_graph* S = slot_of(C, c);
  BatchJob& J = *C.J;
  WbatQuery& Q = C.q[c];
  WtbColumn& K = T.col[c];
  PPRHIP_TRY(read_dead_pops(S, Q.st));
  Q.st.push_ms = K.push_ms;
  Q.st.mc_ms = K.mc_ms;
  Q.st.select_ms = K.sel_ms;
  Q.st.total_ms = host_ms() - Q.t0;
  Q.st.rounds = (int)K.round;
  Q.st.kth_value = K.kth;
  Q.st.rsum = K.rsum;
  Q.st.rmax_final = K.rmax_j;
  Q.st.omega = K.omega_j;
  ForaRun r;
  r.g = S;
  r.query = Q.query;
  r.kind = QueryKind::kTopk;
  r.st = Q.st;
  r.nsel = K.nsel;
  r.ids_out = row_ids(J, Q.query);
  r.vals_out = row_vals(J, Q.query);
  PPRHIP_TRY(deliver_vector(J, r));
  add_stats(J.sum, r.st);
  Q.query = -1;
  return PPRHIP_OK;
}

// Query i begins on column c as weighted_topk_drive begins it on the handle: the workspace reset, the seed table, the
// live seeds as round 0's frontier.  A set without a live seed is over at once: the estimate is p, rounds = 0, one
// selection.
int wtb_begin(WtbCall& T, WbatCall& C, int c, int i) {
  pprhip_graph* S = slot_of(C, c);
  BatchJob& J = *C.J;
  WbatQuery& Q = C.q[c];
  WtbColumn& K = T.col[c];
  Q = WbatQuery();
  K = WtbColumn();
  std::memset(&Q.st, 0, sizeof Q.st);
  S->tun = C.P->tun;
  S->seed_on = false;
  S->topk_active = false;
  SeedTable& plan = J.sets[(size_t)i];
  PPRHIP_TRY(reset_query_state(S, false, plan.max_id));
  PPRHIP_TRY(seed_upload(S, plan));
  PPRHIP_TRY(seed_start(S, Q.L));
  Q.seeded = true;
  Q.query = i;
  Q.t0 = K.t_mark = host_ms();
  K.delta = J.conf->delta;
  K.rsum = J.conf->rsum;
  if (S->seeds->n_live == 0) {
    PPRHIP_CHECK_HIP(hipMemcpyAsync(S->est, S->reserve, sizeof(double) * (size_t)act_n(S), hipMemcpyDeviceToDevice,
                                    S->stream));
    bool have = false;
    PPRHIP_TRY(select_topk(S, S->est, T.k, row_ids(J, i), row_vals(J, i), J.k, &K.nsel, &K.kth, &have, Q.st));
    K.rsum = 0.0;
    K.sel_ms = host_ms() - K.t_mark;
    return wtb_deliver(T, C, c);
  }
  Q.live = true;
  wtb_round_params(T, C, c);
  return PPRHIP_OK;
}

int wtb_rounds(WbatCall& C, void* arg) {
  WtbCall& T = *static_cast<WtbCall*>(arg);
  pprhip_graph* P = C.P;
  BatchState* bs = P->batch;
  BatchJob& J = *C.J;
  for (;;) {
    // 4. (first: the call's start) a free column takes the call's next query
    int busy = 0;
    for (int c = 0; c < C.n_cols; ++c) {
      while (C.q[c].query < 0 && C.next < J.q) PPRHIP_TRY(wtb_begin(T, C, c, C.next++));
      busy += C.q[c].query >= 0 ? 1 : 0;
    }
    if (!busy) return PPRHIP_OK;
    // 1. one level of every column with a frontier: run_weighted_levels' rule on the query's own frontier
    bool dense[kBatch] = {};
    bool leveled[kBatch] = {};
    const unsigned long long* cells[kBatch] = {};
    int n_dense = 0;
    for (int c = 0; c < C.n_cols; ++c) {
      WbatQuery& Q = C.q[c];
      if (Q.query < 0 || T.col[c].step != WtbColumn::kLevels || Q.L.nf == 0) continue;
      leveled[c] = true;
      if ((unsigned long long)Q.L.nf + Q.L.ef >= C.dense_thresh) {
        dense[c] = true;
        n_dense++;
      } else {
        PPRHIP_TRY(wbat_sparse_level(C, c, &cells[c]));
      }
    }
    if (n_dense) PPRHIP_TRY(wbat_sweep(C, dense, n_dense));
    // 2. the walk phase of every column whose frontier has emptied: plan, one merged walk launch, selection
    pprhip_graph* walk_cols[kBatch] = {};
    uint64_t walk_seeds[kBatch] = {};
    uint32_t walk_streams[kBatch] = {};
    double* walk_targets[kBatch] = {};
    int n_walk = 0;
    const double t_walk = host_ms();
    for (int c = 0; c < C.n_cols; ++c) {
      WbatQuery& Q = C.q[c];
      WtbColumn& K = T.col[c];
      if (Q.query < 0 || K.step != WtbColumn::kLevels || leveled[c]) continue;
      pprhip_graph* S = slot_of(C, c);
      if (Q.L.prepared) {  // (the last level was a dense one: its column holds zeros but for the rows the sweep does not write)
        PPRHIP_TRY(launch_wbat_leave(S, Q.a.src));
        Q.L.prepared = false;
      }
      // est := reserve, then the plan of the top-k rounds, its budget derived on the device
      PPRHIP_TRY(launch_sum_partial(S, S->residue, act_n(S)));
      PPRHIP_TRY(launch_walk_plan(S, 1, C.alpha, 0.0, 0, S->est, K.omega_j, S->reserve, S->est));
      walk_cols[c] = S;
      walk_seeds[c] = J.seed + (uint64_t)Q.query;
      walk_streams[c] = K.round;
      walk_targets[c] = S->est;
      K.push_ms += t_walk - K.t_mark;
      n_walk++;
    }
    if (n_walk) {
      ktimer().begin(PPRHIP_KERNEL_WALK, 0);  // (its bytes are added when the counters are read)
      PPRHIP_TRY(launch_w_walk_multi(P, walk_cols, walk_seeds, walk_streams, walk_targets, C.alpha));
      ktimer().end();
      for (int c = 0; c < C.n_cols; ++c)
        if (walk_cols[c]) PPRHIP_TRY(select_launch(walk_cols[c], walk_cols[c]->est, T.k, &T.col[c].sel_seq, true));
    }
    // 3. the selections, the columns' decisions, and the round's one read-back of counters
    const double t_sel = host_ms();
    for (int c = 0; c < C.n_cols; ++c) {
      if (!walk_cols[c]) continue;
      pprhip_graph* S = walk_cols[c];
      WbatQuery& Q = C.q[c];
      WtbColumn& K = T.col[c];
      bool have = false;
      PPRHIP_TRY(select_finish(S, K.sel_seq, S->est, T.k, row_ids(J, Q.query), row_vals(J, Q.query), J.k, &K.nsel, &K.kth,
                               &have, Q.st));
      K.rsum = S->sel_plan_sum;  // (the residue sum this round's plan was derived from)
      if (!have) K.kth = 0.0;
      K.round++;
      const double t_end = host_ms();
      K.mc_ms += t_sel - t_walk;
      K.sel_ms += t_end - t_sel;
      K.t_mark = t_end;
      if (T.sc.last(K.kth, K.delta)) {
        PPRHIP_TRY(wtb_deliver(T, C, c));
        continue;
      }
      // the next round: every node active at its threshold (possibly none: straight to the walks)
      K.delta = T.sc.next(K.delta);
      wtb_round_params(T, C, c);
      Q.L = WLevels();
      unsigned long long* const cell = &S->ctr->hist[0];
      PPRHIP_CHECK_HIP(hipMemsetAsync(cell, 0, sizeof(unsigned long long), S->stream));
      {
        SetupScope setup(S);
        PPRHIP_TRY(launch_wq_collect(S, K.rmax_j, Q.L.fcur, cell));
      }
      cells[c] = cell;
      K.step = WtbColumn::kCollect;
    }
    bool waiting = false;
    for (int c = 0; c < C.n_cols; ++c)
      waiting = waiting || (C.q[c].query >= 0 && (leveled[c] || T.col[c].step == WtbColumn::kCollect));
    if (!waiting) continue;
    PPRHIP_TRY(launch_wbat_collect(P, cells));
    PPRHIP_TRY(fetch_small(P, bs->sweep_out, bs->h_sweep_out, sizeof(unsigned long long) * kBatch));
    for (int c = 0; c < C.n_cols; ++c) {
      WbatQuery& Q = C.q[c];
      if (Q.query < 0 || !(leveled[c] || T.col[c].step == WtbColumn::kCollect)) continue;
      const unsigned long long pk = bs->h_sweep_out[c];
      Q.L.nf = (uint32_t)(pk >> kPackShift);
      Q.L.ef = pk & kPackMask;
      Q.st.enqueues += Q.L.nf;
      T.col[c].step = WtbColumn::kLevels;
    }
  }
}

// The job J (checked; its queries are the seed tables J.sets) on the handle's batch workspaces.
int wtb_run(pprhip_graph_t* g, BatchJob& J, pprhip_stats_t* stats_sum) {
  WbatCall* Cp = new (std::nothrow) WbatCall();
  WtbCall* Tp = new (std::nothrow) WtbCall();
  int rc = PPRHIP_ERR_OOM;
  if (Cp && Tp) {
    Tp->sc = TopkSchedule(J.eps * 0.5, J.conf);
    Tp->k = J.conf->k;
    rc = wbat_run(g, J, *Cp, wtb_rounds, Tp, "batched weighted top-k", stats_sum);
  }
  delete Cp;
  delete Tp;
  return rc;
}

// Both entry points behind their checks: J.sets holds the q seed tables.
int weighted_topk_batch(pprhip_graph_t* g, BatchJob& J, int q, double eps, const pprhip_fora_conf_t* conf, uint64_t seed,
                        pprhip_results_t* keep, int32_t* ids_out, double* vals_out, int* n_out,
                        pprhip_stats_t* per_query, pprhip_stats_t* stats_sum) {
  J.P = g;
  J.srcs = nullptr;
  J.q = q;
  J.eps = eps;
  J.conf = conf;
  J.seed = seed;
  J.k = conf->k;
  J.ids_out = ids_out;
  J.vals_out = vals_out;
  J.n_out = n_out;
  J.per_query = per_query;
  J.keep = keep;
  J.kind = QueryKind::kTopk;
  if (keep) keep->count = 0;
  if (q == 0) {
    if (stats_sum) std::memset(stats_sum, 0, sizeof *stats_sum);
    return PPRHIP_OK;
  }
  if (q == 1) {  // a single query never pays a sixteen-column sweep: the single call's loop on the handle's workspace
    pprhip_stats_t st;
    int nsel = 0;
    PPRHIP_TRY(weighted_topk_drive(g, J.sets[0], eps, conf, seed, ids_out, vals_out, J.k, &nsel, nullptr, &st));
    if (n_out) n_out[0] = nsel;
    if (keep) {
      {
        SetupScope setup(g);
        PPRHIP_TRY(launch_copy_f64(g, g->est, keep->buf, (size_t)g->gr->n));
      }
      PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    }
    if (per_query) per_query[0] = st;
    if (stats_sum) *stats_sum = st;
  } else {
    PPRHIP_TRY(wtb_run(g, J, stats_sum));
  }
  if (keep) keep->count = q;
  return PPRHIP_OK;
}

// what both entry points check of their numbers before the handle is looked at
int wtb_check_params(int q, double eps, const pprhip_fora_conf_t* conf, const int32_t* ids_out, const double* vals_out,
                     const char* fn) {
  PPRHIP_TRY(check_positive(eps, fn, "eps"));
  PPRHIP_TRY(check_conf(conf, fn, true));
  if (!conf || conf->k < 1 || q < 0 || (q > 0 && (!ids_out || !vals_out))) {
    set_error("%s: bad arguments (q=%d k=%d)", fn, q, conf ? conf->k : 0);
    return PPRHIP_ERR_INVALID;
  }
  return PPRHIP_OK;
}

}  // namespace

extern "C" {

int pprhip_weighted_fora_batch_topk(pprhip_graph_t* g, const int32_t* srcs, int q, double eps,
                                    const pprhip_fora_conf_t* conf, uint64_t seed, pprhip_results_t* keep,
                                    int32_t* ids_out, double* vals_out, int* n_out, pprhip_stats_t* per_query,
                                    pprhip_stats_t* stats_sum) {
  static const char* fn = "pprhip_weighted_fora_batch_topk";
  PPRHIP_TRY(wtb_check_params(q, eps, conf, ids_out, vals_out, fn));
  if (q > 0 && !srcs) {
    set_error("%s: null sources", fn);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  PPRHIP_TRY(check_keep(keep, g, q, fn));
  for (int i = 0; i < q; ++i) PPRHIP_TRY(check_node(g, srcs[i], fn));
  BatchJob J;
  try {
    J.sets.resize((size_t)q);
    for (int i = 0; i < q; ++i)  // the set {srcs[i]} with weight 1
      PPRHIP_TRY(seed_plan(g, &srcs[i], nullptr, 1, conf->alpha, fn, J.sets[(size_t)i]));
  } catch (const std::exception& ex) {
    set_error("%s: %s", fn, ex.what());
    return PPRHIP_ERR_OOM;
  }
  return weighted_topk_batch(g, J, q, eps, conf, seed, keep, ids_out, vals_out, n_out, per_query, stats_sum);
}

int pprhip_weighted_fora_batch_topk_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights,
                                          const uint64_t* offsets, int q, double eps, const pprhip_fora_conf_t* conf,
                                          uint64_t seed, pprhip_results_t* keep, int32_t* ids_out, double* vals_out,
                                          int* n_out, pprhip_stats_t* per_query, pprhip_stats_t* stats_sum) {
  static const char* fn = "pprhip_weighted_fora_batch_topk_seeds";
  PPRHIP_TRY(wtb_check_params(q, eps, conf, ids_out, vals_out, fn));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  PPRHIP_TRY(check_keep(keep, g, q, fn));
  BatchJob J;
  PPRHIP_TRY(seed_plan_sets(g, seeds, weights, offsets, q, conf->alpha, fn, J.sets));
  return weighted_topk_batch(g, J, q, eps, conf, seed, keep, ids_out, vals_out, n_out, per_query, stats_sum);
}

int pprhip_walk_multi_shares(const uint64_t counts[16], uint32_t base_waves, uint64_t* per_out, uint32_t first_out[17]) {
  static_assert(kBatch == 16, "the C ABI states the table's size");
  if (!counts || !per_out || !first_out || base_waves == 0) {
    set_error("pprhip_walk_multi_shares: bad arguments (base_waves=%u)", base_waves);
    return PPRHIP_ERR_INVALID;
  }
  unsigned long long c[kBatch], per = 0;
  for (int i = 0; i < kBatch; ++i) {
    if (counts[i] > kPackMask) {
      set_error("pprhip_walk_multi_shares: counts[%d] = %llu exceeds the engine's 2^36 walk limit", i,
                (unsigned long long)counts[i]);
      return PPRHIP_ERR_INVALID;
    }
    c[i] = counts[i];
  }
  walk_multi_deal(c, base_waves, &per, first_out);
  *per_out = per;
  return PPRHIP_OK;
}

}  // extern "C"
