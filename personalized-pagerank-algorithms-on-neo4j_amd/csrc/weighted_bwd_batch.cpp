// weighted_bwd_batch.cpp — batched weighted targets (include/pprhip.h "weighted relationships", the backward direction;
// DESIGN.md §2 "Batched weighted targets"): a pprhip_weighted_ppr_targets call of two or more queries runs with up to
// kBatch of them in flight on the handle's batch workspaces, the queries that stand at a dense level sharing one sweep of
// kernels_weighted_bwd_batch.hip.  A lockstep loop like weighted_batch.cpp's, with one read-back per round and one
// difference: while any busy column has a sparse level to run, only those columns run (one level each) and the columns
// at a dense level wait; a sweep runs when every busy column stands at a dense level.  Waiting adds no kernel work and
// no round beyond the longest query's levels, and it lets the dense columns gather in fewer sweeps.  Query i takes,
// level by level, the decisions of the call of that one query (weighted_bwd.cpp: the serial path, which a call of one
// keeps); batching changes the order of additions inside dense levels only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "run.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace {

struct WbbQuery {  // the query a column's workspace is running
  int query = -1;  // index in the call (-1: the column is free)
  WLevels L;       // (L.prepared: the frontier is held as contributions in the column; ccur and dslot go unused)
  PushArgs a{};
  pprhip_stats_t st;
  int32_t lone = -1;   // the single target without in-edges: no level runs, it is the vector's only entry
  bool fresh = false;  // the column holds a scattered list that no sweep has consumed yet
  double t0 = 0.0;     // host clock at the query's begin (ms)
};

struct WbbCall {
  pprhip_graph* P = nullptr;
  BatchJob* J = nullptr;
  const TargetPlan* tp = nullptr;
  unsigned long long dense_thresh = 0;
  int n_cols = kBatch;
  int next = 0;  // the call's next query
  WbbQuery q[kBatch];
};

pprhip_graph* slot_of(const WbbCall& C, int c) { return C.P->batch->slots[(size_t)c]; }

// Query i begins on column c's workspace as the serial path begins it on the handle's: the workspace reset, then the
// start of a single target (r(t) = 1, t the first frontier; without in-edges reserve(t) = alpha and no push) or of a
// set (k_target_init; its first frontier is known to the host).
int wbb_begin(WbbCall& C, int c, int i) {
  pprhip_graph* S = slot_of(C, c);
  const TargetPlan& tp = *C.tp;
  WbbQuery& Q = C.q[c];
  Q = WbbQuery();
  std::memset(&Q.st, 0, sizeof Q.st);
  S->tun = C.P->tun;
  S->seed_on = false;
  S->topk_active = false;
  const int32_t single = tp.single[(size_t)i];
  PPRHIP_TRY(reset_query_state(S, false, tp.max_id[(size_t)i]));
  Q.a = PushArgs{tp.alpha, tp.rmax, 0.0, single, kBackward};
  Q.t0 = host_ms();
  if (single >= 0) {
    const uint32_t d = hdeg_in(S, single);
    if (d == 0) {
      Q.lone = single;
      PPRHIP_TRY(launch_set_f64(S, S->reserve, (uint32_t)single, tp.alpha));
    } else {
      PPRHIP_TRY(launch_set_f64(S, S->residue, (uint32_t)single, 1.0));
      PPRHIP_TRY(launch_seed_one(S, Q.L.fcur, single));
      Q.L.nf = 1;
      Q.L.ef = d;
    }
  } else {
    // (the counter is zero: reset_query_state cleared the counters)
    PPRHIP_TRY(launch_target_init(S, tp.d_id + tp.first[(size_t)i], tp.d_w + tp.first[(size_t)i], tp.count[(size_t)i],
                                  Q.L.fcur, &S->ctr->hist[kMaxBatch + 2], tp.alpha, tp.rmax));
    Q.L.nf = tp.nf[(size_t)i];
    Q.L.ef = tp.ef[(size_t)i];
  }
  Q.query = i;
  return PPRHIP_OK;
}

// The query's push is over (its column holds zeros: the last sweep left no crossing, or the last compaction emptied
// it): value = p / S_w in place of the reserve, then the delivery.  The column is free afterwards.
int wbb_finish(WbbCall& C, int c) {
  pprhip_graph* S = slot_of(C, c);
  BatchJob& J = *C.J;
  WbbQuery& Q = C.q[c];
  Q.st.push_ms = host_ms() - Q.t0;  // the host's clock: the workspace shares its stream with the other columns
  PPRHIP_TRY(launch_target_finish(S, C.tp->survival, act_n(S), Q.lone));
  Q.st.rmax_final = C.tp->rmax;
  Q.st.rounds = 1;
  Q.st.total_ms = host_ms() - Q.t0;
  ForaRun r;
  r.g = S;
  r.query = Q.query;
  r.kind = QueryKind::kTargets;
  r.st = Q.st;
  PPRHIP_TRY(deliver_vector(J, r));
  add_stats(J.sum, r.st);
  Q.query = -1;
  return PPRHIP_OK;
}

// One sparse level of column c's query on its own workspace: run_weighted_levels' sparse branch (backward) without its
// read-back (the round's collect brings the counter).  *cell: where the level leaves the next frontier's counter.
int wbb_sparse_level(WbbCall& C, int c, const unsigned long long** cell) {
  pprhip_graph* S = slot_of(C, c);
  WbbQuery& Q = C.q[c];
  WLevels& L = Q.L;
  unsigned long long* const list_counter = &S->ctr->hist[1];
  uint32_t nf_list = L.nf;
  uint64_t ef_list = L.ef;
  const uint64_t bytes = 36ull * L.nf + 44ull * L.ef;
  ktimer().begin(PPRHIP_KERNEL_SPARSE_PUSH, bytes);
  if (L.prepared) {  // the column -> list, recounted as the serial path recounts it
    PPRHIP_CHECK_HIP(hipMemsetAsync(&S->ctr->hist[0], 0, 2 * sizeof(unsigned long long), S->stream));
    PPRHIP_TRY(launch_wbb_compact(S, L.fcur, &S->ctr->hist[0]));
    PPRHIP_TRY(fetch_packed(S, &S->ctr->hist[0], &nf_list, &ef_list));
    L.prepared = false;
  } else {
    PPRHIP_TRY(launch_wb_prepare(S, Q.a, L.fcur, L.nf, false, 0, list_counter));
  }
  PPRHIP_TRY(launch_wb_push(S, Q.a, L.fcur, nf_list, ef_list, list_counter));
  ktimer().end();
  Q.st.pops += L.nf;
  Q.st.edge_pushes += L.ef;
  Q.st.levels++;
  Q.st.push_bytes += bytes;
  L.fcur ^= 1;
  *cell = list_counter;
  return PPRHIP_OK;
}

// The sweep of the columns in `dense`: their lists scattered, their arguments staged, the kernels, the members without
// out-edges taken out of a column that was just scattered, the level bookkeeping of their queries.
int wbb_sweep(WbbCall& C, const bool* dense, int n_dense) {
  pprhip_graph* P = C.P;
  BatchState* bs = P->batch;
  const GraphData* D = P->gr;
  for (int c = 0; c < kBatch; ++c) {
    SlotArgs& sa = bs->h_slot_args[c];
    std::memset(&sa, 0, sizeof sa);
    if (!dense[c]) continue;
    pprhip_graph* S = slot_of(C, c);
    WbbQuery& Q = C.q[c];
    if (!Q.L.prepared) {  // list form -> the column
      PPRHIP_TRY(launch_wbb_scatter(S, Q.a, Q.L.fcur, Q.L.nf));
      Q.L.prepared = true;
      Q.fresh = true;
    }
    sa.res = S->residue;
    sa.reserve = S->reserve;
    sa.ctr = S->ctr;
    sa.alpha = Q.a.alpha;
    sa.rmax = Q.a.rmax;
    sa.src = Q.a.src;
    sa.active = 1;
    sa.mode = kBackward;
    sa.out_slot = Q.L.pslot ^ 1;
  }
  // out_ci and out_w once for all columns; per column the gathers and the rows' work
  const uint64_t bytes = 12ull * D->m + (uint64_t)n_dense * (8ull * D->m + 40ull * D->n_nz_o);
  ktimer().begin(PPRHIP_KERNEL_DENSE_PULL_BATCH, bytes);
  PPRHIP_TRY(launch_wbb_sweep(P));
  ktimer().end();
  const uint64_t level_bytes = 12ull * D->m + 8ull * D->m + 40ull * D->n_nz_o;  // what the serial path charges a dense level
  for (int c = 0; c < kBatch; ++c)
    if (dense[c]) {
      WbbQuery& Q = C.q[c];
      if (Q.fresh) {  // (the list the scatter read is still in F[fcur]: dense levels leave the lists alone)
        PPRHIP_TRY(launch_wbb_leave(slot_of(C, c), Q.L.fcur, Q.L.nf));
        Q.fresh = false;
      }
      Q.st.dense_levels++;
      Q.st.levels++;
      Q.st.dense_nodes += Q.L.nf;
      Q.st.dense_edges += Q.L.ef;
      Q.st.push_bytes += level_bytes;
      Q.L.pslot ^= 1;
    }
  return PPRHIP_OK;
}

int wbb_rounds(WbbCall& C) {
  pprhip_graph* P = C.P;
  BatchState* bs = P->batch;
  for (;;) {
    int busy = 0;
    for (int c = 0; c < C.n_cols; ++c) {
      WbbQuery& Q = C.q[c];
      for (;;) {  // (a target without in-edges is finished as soon as it has begun)
        if (Q.query >= 0 && Q.L.nf == 0) PPRHIP_TRY(wbb_finish(C, c));
        if (Q.query >= 0 || C.next >= C.J->q) break;
        PPRHIP_TRY(wbb_begin(C, c, C.next++));
      }
      busy += Q.query >= 0 ? 1 : 0;
    }
    if (!busy) return PPRHIP_OK;
    // the rule of run_weighted_levels on every query's own frontier; the columns at a sparse level go first
    bool dense[kBatch] = {}, ran[kBatch] = {};
    const unsigned long long* cells[kBatch] = {};
    int n_dense = 0, n_sparse = 0;
    for (int c = 0; c < C.n_cols; ++c) {
      const WbbQuery& Q = C.q[c];
      if (Q.query < 0) continue;
      dense[c] = (unsigned long long)Q.L.nf + Q.L.ef >= C.dense_thresh;
      n_dense += dense[c] ? 1 : 0;
      n_sparse += dense[c] ? 0 : 1;
    }
    if (n_sparse) {
      for (int c = 0; c < C.n_cols; ++c)
        if (C.q[c].query >= 0 && !dense[c]) {
          PPRHIP_TRY(wbb_sparse_level(C, c, &cells[c]));
          ran[c] = true;
        }
    } else {
      PPRHIP_TRY(wbb_sweep(C, dense, n_dense));
      for (int c = 0; c < C.n_cols; ++c) ran[c] = dense[c];
    }
    PPRHIP_TRY(launch_wbat_collect(P, cells));
    PPRHIP_TRY(fetch_small(P, bs->sweep_out, bs->h_sweep_out, sizeof(unsigned long long) * kBatch));
    for (int c = 0; c < C.n_cols; ++c) {
      if (!ran[c]) continue;  // (a column that waited keeps its frontier: its cell of sweep_out was not written)
      WbbQuery& Q = C.q[c];
      const unsigned long long pk = bs->h_sweep_out[c];
      Q.L.nf = (uint32_t)(pk >> kPackShift);
      Q.L.ef = pk & kPackMask;
      Q.st.enqueues += Q.L.nf;
    }
  }
}

}  // namespace

int pprhip::detail::weighted_targets_batch(pprhip_graph_t* g, const TargetPlan& tp, int q, pprhip_results* keep,
                                           double* values_out, int k, int32_t* ids_out, double* vals_out, int* n_out,
                                           pprhip_stats_t* per_query, pprhip_stats_t* stats_sum) {
  PPRHIP_TRY(ensure_batch(g));
  PPRHIP_TRY(ensure_bwd_layout(g));
  BatchState* bs = g->batch;
  BatchJob J;
  J.P = g;
  J.kind = QueryKind::kTargets;
  J.q = q;
  J.reserve_out = values_out;
  J.k = k;
  J.ids_out = ids_out;
  J.vals_out = vals_out;
  J.n_out = n_out;
  J.per_query = per_query;
  J.keep = keep;
  if (keep) keep->count = 0;
  WbbCall* Cp = new (std::nothrow) WbbCall();
  if (!Cp) return PPRHIP_ERR_OOM;
  WbbCall& C = *Cp;
  C.P = g;
  C.J = &J;
  C.tp = &tp;
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
  g->topk_active = false;
  g->ktimer.stream = g->stream;
  g->ktimer.reset();
  const double t0 = host_ms();
  KernelTimer local;  // (the caller's timer may be in use)
  KernelTimer* const saved = g_timer_cur;
  g_timer_cur = &local;
  local.stream = g->stream;
  int rc = PPRHIP_OK;
  // A column nobody owns holds zeros, in both arrays (the calls before may have left entries on rows this sweep does
  // not rewrite), and the row sums are all-zero in the backward layout: an unweighted forward call or a batched weighted
  // FORA call before may have left sums in the other one.
  const size_t c8_bytes = sizeof(double) * (size_t)g->gr->n * kBatch;
  if (hipMemsetAsync(bs->c8[0], 0, c8_bytes, g->stream) != hipSuccess ||
      hipMemsetAsync(bs->c8[1], 0, c8_bytes, g->stream) != hipSuccess ||
      (bs->acc8_dir != 1 &&
       hipMemsetAsync(bs->acc8, 0, sizeof(double) * ((size_t)g->gr->n + 1) * kBatch, g->stream) != hipSuccess)) {
    set_error("batched weighted targets: clearing the shared arrays failed: %s", hipGetErrorString(hipGetLastError()));
    rc = PPRHIP_ERR_HIP;
  }
  bs->acc8_dir = 1;
  if (rc == PPRHIP_OK) rc = wbb_rounds(C);
  const std::string msg = rc != PPRHIP_OK ? get_error() : std::string();
  (void)hipStreamSynchronize(g->stream);
  double tot[8] = {0};
  uint64_t bytes[8] = {0};
  uint32_t cnt[8] = {0};
  local.resolve(tot, bytes, cnt);
  local.destroy();
  g_timer_cur = saved;
  delete Cp;
  if (rc != PPRHIP_OK) {
    free_batch(g);  // workspaces may hold half-pushed levels: the next batched call builds clean ones
    set_error("%s", msg.c_str());
    return rc;
  }
  J.sum.total_ms = host_ms() - t0;
  fold_class_totals(J.sum, tot, bytes, cnt);
  if (keep) keep->count = q;
  if (stats_sum) {
    J.sum.rmax_final = tp.rmax;
    *stats_sum = J.sum;
  }
  return PPRHIP_OK;
}
