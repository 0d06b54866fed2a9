// weighted_batch.cpp — batched weighted FORA (include/pprhip.h "batched weighted FORA"): up to kBatch
// weighted whole-graph queries in flight on the handle's batch workspaces, their dense levels sharing one sweep of
// kernels_weighted_batch.hip.  The weighted level loop is plain frontier-synchronous Jacobi with one host round trip per
// level (weighted.cpp: run_weighted_levels), so the driver is a lockstep loop: per round every live query below the
// dense threshold runs one sparse level on its own workspace with the single-query kernels, the others share one
// batched sweep, and one read-back brings every counter.  A query whose frontier is empty runs its walk phase and its
// delivery on its workspace, which then takes the call's next query.  Query i takes, level by level, the decisions of
// pprhip_weighted_fora(srcs[i]) / pprhip_weighted_fora_seeds(set i); batching changes the order of additions only.
// One level of a column, the shared sweep and the call's bring-up (weighted_batch.hpp) also serve the batched weighted
// top-k driver (weighted_topk_batch.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "weighted_batch.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace pprhip {
namespace detail {

// One sparse level of column c's query on its own workspace: run_weighted_levels' sparse branch without its read-back
// (the round's collect brings the counter).  *cell: where the level leaves the next frontier's counter.
int wbat_sparse_level(WbatCall& C, int c, const unsigned long long** cell) {
  pprhip_graph* S = slot_of(C, c);
  WbatQuery& Q = C.q[c];
  WLevels& L = Q.L;
  unsigned long long* const list_counter = &S->ctr->hist[1];
  uint32_t nf_list = L.nf;
  uint64_t ef_list = L.ef;
  const uint64_t bytes = 44ull * L.nf + 36ull * L.ef;
  ktimer().begin(PPRHIP_KERNEL_SPARSE_PUSH, bytes);
  if (L.prepared) {
    // the column -> list (dead-end nodes carry no contribution: the list is recounted; it may be empty while their mass
    // still has to land, so the level runs whatever the recount says)
    PPRHIP_CHECK_HIP(hipMemsetAsync(&S->ctr->hist[0], 0, 2 * sizeof(unsigned long long), S->stream));
    PPRHIP_TRY(launch_wbat_compact(S, L.fcur, &S->ctr->hist[0]));
    PPRHIP_TRY(launch_wbat_leave(S, Q.a.src));
    PPRHIP_TRY(fetch_packed(S, &S->ctr->hist[0], &nf_list, &ef_list));
    L.prepared = false;
  } else {
    PPRHIP_TRY(launch_w_prepare(S, Q.a, L.fcur, L.nf, false, 0, L.dslot, list_counter));
  }
  if (Q.seeded) PPRHIP_TRY(launch_wq_land_sparse(S, Q.a, L.fcur, L.dslot, list_counter));
  PPRHIP_TRY(launch_w_push(S, Q.a, L.fcur, nf_list, ef_list, L.dslot, list_counter));
  ktimer().end();
  Q.st.pops += L.nf;
  Q.st.edge_pushes += L.ef;
  Q.st.levels++;
  Q.st.push_bytes += bytes;
  L.fcur ^= 1;
  *cell = list_counter;
  return PPRHIP_OK;
}

// The sweep of the columns in `dense`: their arguments staged, the kernels, the level bookkeeping of their queries.
int wbat_sweep(WbatCall& C, const bool* dense, int n_dense) {
  pprhip_graph* P = C.P;
  BatchState* bs = P->batch;
  const GraphData* D = P->gr;
  int n_seeded = 0;
  for (int c = 0; c < kBatch; ++c) {
    SlotArgs& sa = bs->h_slot_args[c];
    std::memset(&sa, 0, sizeof sa);
    if (!dense[c]) continue;
    pprhip_graph* S = slot_of(C, c);
    WbatQuery& Q = C.q[c];
    if (!Q.L.prepared) {  // list form -> the column
      PPRHIP_TRY(launch_wbat_scatter(S, Q.a, Q.L.fcur, Q.L.nf, Q.L.dslot));
      Q.L.prepared = true;
    }
    sa.res = S->residue;
    sa.reserve = S->reserve;
    sa.ctr = S->ctr;
    sa.alpha = Q.a.alpha;
    sa.rmax = Q.a.rmax;
    sa.src = Q.a.src;
    sa.active = 1;
    sa.mode = kFwdWhole;
    sa.dead_slot = Q.L.dslot;
    sa.out_slot = Q.L.pslot ^ 1;
    sa.gs_state = kGsJacobi;
    if (Q.seeded) {
      sa.seed_w = S->seeds->w_node;
      n_seeded++;
    }
  }
  // in_ci and in_w once for all columns; per column the gathers and the rows' work (+ a seeded column's landing weights)
  const uint64_t bytes = 12ull * D->m + (uint64_t)n_dense * (8ull * D->m + 40ull * D->n_nz) + (uint64_t)n_seeded * 8ull * D->n_nz;
  ktimer().begin(PPRHIP_KERNEL_DENSE_PULL_BATCH, bytes);
  PPRHIP_TRY(launch_wbat_sweep(P));
  ktimer().end();
  const uint64_t level_bytes = 12ull * D->m + 8ull * D->m + 40ull * D->n_nz;  // what the single call charges a dense level
  for (int c = 0; c < kBatch; ++c)
    if (dense[c]) {
      WbatQuery& Q = C.q[c];
      Q.st.dense_levels++;
      Q.st.levels++;
      Q.st.dense_nodes += Q.L.nf;
      Q.st.dense_edges += Q.L.ef;
      Q.st.push_bytes += level_bytes;
      Q.L.dslot ^= 1;
      Q.L.pslot ^= 1;
    }
  return PPRHIP_OK;
}

// A batched weighted call's bring-up and its end around `rounds` (the call's driver loop): the batch state, C filled
// but for what only the caller knows (rmax, omega), the workspaces on the handle's stream, a timer of the call's own,
// the shared arrays cleared; afterwards the class totals into J.sum and stats_sum, or - after an error - free_batch and
// the message kept.  `what` names the call in the messages.
int wbat_run(pprhip_graph_t* g, BatchJob& J, WbatCall& C, int (*rounds)(WbatCall&, void*), void* arg, const char* what,
             pprhip_stats_t* stats_sum) {
  PPRHIP_TRY(ensure_batch(g));
  BatchState* bs = g->batch;
  C.P = g;
  C.J = &J;
  C.alpha = J.conf->alpha;
  C.dense_thresh = (unsigned long long)std::ceil(g->tun.dense_frac * (double)g->gr->m);
  // one column per batch workspace: fewer than kBatch when the handle is told to keep fewer
  C.n_cols = (int)std::min<size_t>((size_t)kBatch, bs->slots.size());
  if (const char* e = tuning_env("PPRHIP_BATCH_WORKSPACES")) C.n_cols = std::max(1, std::min(C.n_cols, atoi(e)));
  for (pprhip_graph* S : bs->slots) {
    S->stream = g->stream;
    S->c8_via_parent = false;
    S->sync = nullptr;
  }
  if (bs->share) bs->share->on = false;  // (the unweighted calls' terminal cache)
  std::memset(&J.sum, 0, sizeof J.sum);
  g->ktimer.stream = g->stream;
  g->ktimer.reset();
  const double t0 = host_ms();
  KernelTimer local;  // (the caller's timer may be in use)
  KernelTimer* const saved = g_timer_cur;
  g_timer_cur = &local;
  local.stream = g->stream;
  int rc = PPRHIP_OK;
  // A column nobody owns holds zeros, in both arrays: the calls before may have left entries on rows this sweep does
  // not rewrite (an unweighted sweep's rows without in-edges, a backward call's entry preparation), and row sums in the
  // other layout.
  const size_t c8_bytes = sizeof(double) * (size_t)g->gr->n * kBatch;
  if (hipMemsetAsync(bs->c8[0], 0, c8_bytes, g->stream) != hipSuccess ||
      hipMemsetAsync(bs->c8[1], 0, c8_bytes, g->stream) != hipSuccess ||
      (bs->acc8_dir != 0 &&
       hipMemsetAsync(bs->acc8, 0, sizeof(double) * ((size_t)g->gr->n + 1) * kBatch, g->stream) != hipSuccess)) {
    set_error("%s: clearing the shared arrays failed: %s", what, hipGetErrorString(hipGetLastError()));
    rc = PPRHIP_ERR_HIP;
  }
  bs->acc8_dir = 0;
  try {
    if (rc == PPRHIP_OK) rc = rounds(C, arg);
  } catch (const std::exception& ex) {  // (no exception may cross the C ABI: the seed tables' vectors allocate)
    set_error("%s: %s", what, ex.what());
    rc = PPRHIP_ERR_OOM;
  }
  const std::string msg = rc != PPRHIP_OK ? get_error() : std::string();
  (void)hipStreamSynchronize(g->stream);
  double tot[8] = {0};
  uint64_t bytes[8] = {0};
  uint32_t cnt[8] = {0};
  local.resolve(tot, bytes, cnt);
  local.destroy();
  g_timer_cur = saved;
  if (rc != PPRHIP_OK) {
    free_batch(g);  // workspaces may hold half-pushed levels and seed tables: the next batched call builds clean ones
    set_error("%s", msg.c_str());
    return rc;
  }
  J.sum.total_ms = host_ms() - t0;
  fold_class_totals(J.sum, tot, bytes, cnt);
  if (stats_sum) *stats_sum = J.sum;
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip

namespace {

// Query i begins on column c's workspace as weighted_fora begins it on the handle's (forward_calls.cpp): the workspace
// reset, the plan installed, the first frontier - none for a dead-end source (reserve = e_s) or a set without a live
// seed (reserve = p).
int wbat_begin(WbatCall& C, int c, int i) {
  pprhip_graph* S = slot_of(C, c);
  BatchJob& J = *C.J;
  WbatQuery& Q = C.q[c];
  Q = WbatQuery();
  std::memset(&Q.st, 0, sizeof Q.st);
  S->tun = C.P->tun;
  S->seed_on = false;
  S->topk_active = false;
  SeedTable* plan = J.srcs ? nullptr : &J.sets[(size_t)i];
  const int32_t src = plan ? -1 : C.P->gr->h_old2new[J.srcs[i]];
  PPRHIP_TRY(reset_query_state(S, false, plan ? plan->max_id : src));
  if (plan) PPRHIP_TRY(seed_upload(S, *plan));
  Q.a = PushArgs{C.alpha, C.rmax, 0.0, src, kFwdWhole};
  Q.seeded = plan != nullptr;
  Q.t0 = host_ms();
  if (plan) {
    PPRHIP_TRY(seed_start(S, Q.L));
    S->seed_on = true;  // (until the query's pushes are over)
  } else {
    const uint32_t d = hdeg_out(S, src);
    if (d == 0) {
      PPRHIP_TRY(launch_set_f64(S, S->reserve, (uint32_t)src, 1.0));
    } else {
      PPRHIP_TRY(launch_set_f64(S, S->residue, (uint32_t)src, 1.0));
      PPRHIP_TRY(launch_seed_one(S, Q.L.fcur, src));
      Q.L.nf = 1;
      Q.L.ef = d;
    }
  }
  Q.live = Q.L.nf != 0;
  Q.query = i;
  return PPRHIP_OK;
}

// The query's push is over: the walk phase of weighted_fora on its workspace (the same plan, the same walks - the
// call's seed, stream 0, forced first hop; served from the weighted walk index as the single call is), the dead-end
// pops, the delivery.  The column is free afterwards.
int wbat_finish(WbatCall& C, int c) {
  pprhip_graph* S = slot_of(C, c);
  BatchJob& J = *C.J;
  WbatQuery& Q = C.q[c];
  if (Q.L.prepared) {  // (the last level was a dense one: its column holds zeros but for the rows the sweep does not write)
    PPRHIP_TRY(launch_wbat_leave(S, Q.a.src));
    Q.L.prepared = false;
  }
  S->seed_on = false;
  double sum = 0.0;
  if (Q.live) PPRHIP_TRY(device_sum(S, S->residue, &sum));
  const double t1 = host_ms();
  const double rsum = sum * (1 - C.alpha);
  if (Q.live) {
    const double nrw_d = C.omega * rsum;
    const long long nrw = (nrw_d == nrw_d && nrw_d > 0.0) ? (long long)nrw_d : 0;
    PPRHIP_TRY(launch_walk_plan(S, 0, C.alpha, rsum, nrw, S->reserve, 0.0));
    ktimer().begin(PPRHIP_KERNEL_WALK, 0);
    PPRHIP_TRY(launch_w_walk_run(S, C.alpha, J.seed, S->reserve, 0u, true));
    ktimer().end();
  }
  PPRHIP_TRY(read_dead_pops(S, Q.st));
  const double t2 = host_ms();
  Q.st.rounds = 1;
  Q.st.rsum = rsum;
  Q.st.rmax_final = C.rmax;
  Q.st.omega = C.omega;
  Q.st.push_ms = t1 - Q.t0;  // the host's clock: the workspace shares its stream with the other columns
  Q.st.mc_ms = t2 - t1;
  Q.st.total_ms = t2 - Q.t0;
  ForaRun r;
  r.g = S;
  r.query = Q.query;
  r.kind = QueryKind::kFora;
  r.st = Q.st;
  PPRHIP_TRY(deliver_vector(J, r));
  add_stats(J.sum, r.st);
  Q.query = -1;
  return PPRHIP_OK;
}

int wbat_rounds(WbatCall& C) {
  pprhip_graph* P = C.P;
  BatchState* bs = P->batch;
  for (;;) {
    int busy = 0;
    for (int c = 0; c < C.n_cols; ++c) {
      WbatQuery& Q = C.q[c];
      for (;;) {  // (a dead-end source is finished as soon as it has begun)
        if (Q.query >= 0 && Q.L.nf == 0) PPRHIP_TRY(wbat_finish(C, c));
        if (Q.query >= 0 || C.next >= C.J->q) break;
        PPRHIP_TRY(wbat_begin(C, c, C.next++));
      }
      busy += Q.query >= 0 ? 1 : 0;
    }
    if (!busy) return PPRHIP_OK;
    // one level of every live query: the rule of run_weighted_levels on the query's own frontier
    bool dense[kBatch] = {};
    const unsigned long long* cells[kBatch] = {};
    int n_dense = 0;
    for (int c = 0; c < C.n_cols; ++c) {
      WbatQuery& Q = C.q[c];
      if (Q.query < 0) continue;
      if ((unsigned long long)Q.L.nf + Q.L.ef >= C.dense_thresh) {
        dense[c] = true;
        n_dense++;
      } else {
        PPRHIP_TRY(wbat_sparse_level(C, c, &cells[c]));
      }
    }
    if (n_dense) PPRHIP_TRY(wbat_sweep(C, dense, n_dense));
    PPRHIP_TRY(launch_wbat_collect(P, cells));
    PPRHIP_TRY(fetch_small(P, bs->sweep_out, bs->h_sweep_out, sizeof(unsigned long long) * kBatch));
    for (int c = 0; c < C.n_cols; ++c) {
      WbatQuery& Q = C.q[c];
      if (Q.query < 0) continue;
      const unsigned long long pk = bs->h_sweep_out[c];
      Q.L.nf = (uint32_t)(pk >> kPackShift);
      Q.L.ef = pk & kPackMask;
      Q.st.enqueues += Q.L.nf;
    }
  }
}

// The job J (checked) on the handle's batch workspaces.
int weighted_batch_run(pprhip_graph_t* g, BatchJob& J, double rmax, pprhip_stats_t* stats_sum) {
  double rmax0 = 0.0, omega = 0.0;
  PPRHIP_TRY(pprhip_fora_whole_params(J.conf, J.eps, &rmax0, &omega));
  WbatCall* Cp = new (std::nothrow) WbatCall();
  if (!Cp) return PPRHIP_ERR_OOM;
  Cp->rmax = rmax == 0.0 ? rmax0 : rmax;
  Cp->omega = omega;
  const int rc = wbat_run(g, J, *Cp, [](WbatCall& C, void*) { return wbat_rounds(C); }, nullptr, "batched weighted FORA",
                          stats_sum);
  delete Cp;
  return rc;
}

// what both entry points check behind the parameters, the handle and the weights
int check_batch_args(int q, int k, const int32_t* ids_out, const double* vals_out, const char* fn) {
  if (q < 0 || k < 0 || (k > 0 && q > 0 && (!ids_out || !vals_out))) {
    set_error("%s: bad arguments (q=%d k=%d)", fn, q, k);
    return PPRHIP_ERR_INVALID;
  }
  return PPRHIP_OK;
}

int weighted_fora_batch(pprhip_graph_t* g, BatchJob& J, const int32_t* srcs, int q, double eps,
                        const pprhip_fora_conf_t* conf, uint64_t seed, double rmax, pprhip_results_t* keep,
                        double* reserve_out, int k, int32_t* ids_out, double* vals_out, int* n_out,
                        pprhip_stats_t* per_query, pprhip_stats_t* stats_sum) {
  J.P = g;
  J.srcs = srcs;
  J.q = q;
  J.eps = eps;
  J.conf = conf;
  J.seed = seed;
  J.reserve_out = reserve_out;
  J.k = k;
  J.ids_out = ids_out;
  J.vals_out = vals_out;
  J.n_out = n_out;
  J.per_query = per_query;
  J.keep = keep;
  if (keep) keep->count = 0;
  if (q == 0) {
    if (stats_sum) std::memset(stats_sum, 0, sizeof *stats_sum);
    return PPRHIP_OK;
  }
  PPRHIP_TRY(weighted_batch_run(g, J, rmax, stats_sum));
  if (keep) keep->count = q;
  return PPRHIP_OK;
}

}  // namespace

extern "C" {

int pprhip_weighted_fora_batch(pprhip_graph_t* g, const int32_t* srcs, int q, double eps, const pprhip_fora_conf_t* conf,
                               uint64_t seed, double rmax, pprhip_results_t* keep, double* reserve_out, int k,
                               int32_t* ids_out, double* vals_out, int* n_out, pprhip_stats_t* per_query,
                               pprhip_stats_t* stats_sum) {
  static const char* fn = "pprhip_weighted_fora_batch";
  PPRHIP_TRY(check_weighted_fora_params(eps, conf, rmax, fn));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  PPRHIP_TRY(check_batch_args(q, k, ids_out, vals_out, fn));
  if (q > 0 && !srcs) {
    set_error("%s: null sources", fn);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_keep(keep, g, q, fn));
  for (int i = 0; i < q; ++i) PPRHIP_TRY(check_node(g, srcs[i], fn));
  BatchJob J;
  return weighted_fora_batch(g, J, srcs, q, eps, conf, seed, rmax, keep, reserve_out, k, ids_out, vals_out, n_out,
                             per_query, stats_sum);
}

int pprhip_weighted_fora_batch_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights,
                                     const uint64_t* offsets, int q, double eps, const pprhip_fora_conf_t* conf,
                                     uint64_t seed, double rmax, pprhip_results_t* keep, double* reserve_out, int k,
                                     int32_t* ids_out, double* vals_out, int* n_out, pprhip_stats_t* per_query,
                                     pprhip_stats_t* stats_sum) {
  static const char* fn = "pprhip_weighted_fora_batch_seeds";
  PPRHIP_TRY(check_weighted_fora_params(eps, conf, rmax, fn));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  PPRHIP_TRY(check_batch_args(q, k, ids_out, vals_out, fn));
  PPRHIP_TRY(check_keep(keep, g, q, fn));
  BatchJob J;
  PPRHIP_TRY(seed_plan_sets(g, seeds, weights, offsets, q, conf->alpha, fn, J.sets));
  return weighted_fora_batch(g, J, nullptr, q, eps, conf, seed, rmax, keep, reserve_out, k, ids_out, vals_out, n_out,
                             per_query, stats_sum);
}

}  // extern "C"
