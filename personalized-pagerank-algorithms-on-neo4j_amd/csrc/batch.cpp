// batch.cpp — the batched entry points' engine: kBatch resumable runs (run.hpp) in flight on the handle's slots, their
// dense levels sharing one sweep.  The sweep's launch / collect, a query's begin / finish, the one-thread driver
// (SlotDriver, batch_driver.hpp) with the leftover rule, the threaded driver (batch_worker, BatchSync) and batch_run.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>

#include "batch_driver.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace pprhip {
namespace detail {

int launch_sweep(pprhip_graph* P, ForaRun* runs, const bool* active, int n_active, SweepTicket* T, const int* ws) {
  BatchState* bs = P->batch;
  const GraphData* D = P->gr;
  T->n_active = n_active;
  int n_seeded = 0;
  for (int s = 0; s < kBatch; ++s) {
    T->ws[s] = (ws && active[s]) ? ws[s] : s;
    pprhip_graph* S = bs->slots[T->ws[s]];
    SlotArgs& sa = bs->h_slot_args[s];
    T->active[s] = active[s];
    sa.res = S->residue;
    sa.reserve = S->reserve;
    sa.flags = S->flags;
    sa.armed = S->armed;
    sa.ctr = S->ctr;
    sa.active = active[s] ? 1 : 0;
    // a seeded query lands its dead-end mass in the sweep (k_dense_apply_batch, k_seed_land_dense_batch)
    const SeedTable* sd = (active[s] && S->seed_on) ? S->seeds : nullptr;
    sa.seed_w = sd ? sd->w_node : nullptr;
    sa.seed_id = sd ? sd->id : nullptr;
    sa.seed_e = sd ? sd->w : nullptr;
    sa.seed_done = sd ? sd->done : nullptr;
    sa.seed_n_live = sd ? sd->n_live : 0u;
    sa.seed_n_all = sd ? sd->n_live + sd->n_dead : 0u;
    n_seeded += sd ? 1 : 0;
    if (!active[s]) continue;
    const ForaRun& r = runs[T->ws[s]];
    sa.alpha = r.a.alpha;
    sa.rmax = r.a.rmax;
    sa.min_rmax = r.a.min_rmax;
    sa.src = r.a.src;
    sa.mode = r.a.mode;
    sa.dead_slot = r.L.dslot;
    sa.out_slot = r.L.pslot ^ 1;
    sa.gs_state = r.L.gs_state;
    // (a slot of the sequential driver has put its prepared level on the parent's stream itself: C8Scope)
    if (S->stream != P->stream && !S->c8_via_parent) {
      PPRHIP_CHECK_HIP(hipEventRecord(S->ev[3], S->stream));
      PPRHIP_CHECK_HIP(hipStreamWaitEvent(P->stream, S->ev[3], 0));
    }
  }
  bool backward = false;
  for (int s = 0; s < kBatch; ++s)
    if (active[s] && runs[T->ws[s]].a.mode == kBackward) backward = true;  // a job's runs all push the same way
  T->backward = backward;
  // SURVEY 8(d) sweep model with n = the rows the sweep carries (launch_dense_level_b8: isolated nodes are left out)
  const uint64_t rows = backward ? (uint64_t)D->n_nz_o + D->n_z_o : (uint64_t)D->n_nz + D->n_zin;
  T->rows = rows;
  // (+ 8 B per row for each seeded column: its landing weights)
  const uint64_t sweep_bytes =
      4ull * D->m + (uint64_t)n_active * (8ull * D->m + 36ull * rows + 4ull) + (uint64_t)n_seeded * 8ull * rows;
  if ((int)backward != bs->acc8_dir) {
    // rows summed with atomics are cleared by the apply kernel of their own layout only: start clean
    PPRHIP_CHECK_HIP(hipMemsetAsync(bs->acc8, 0, sizeof(double) * ((size_t)D->n + 1) * kBatch, P->stream));
    bs->acc8_dir = (int)backward;
  }
  int n_gs = 1;
  const GsBlock* gs_blocks = backward ? nullptr : gs_blocks_of(bs->slots[0], &n_gs);  // slots carry the call's tuning
  // (Tried against the ~30 us between two sweeps, round 5: the slots' arguments passed to the kernels by value instead
  // of through a copy command, and the reduce kernel writing the counters into the mailbox itself instead of a
  // k_publish behind it - the sweep took 20-35 us longer either way (1 636-1 651 against 1 613-1 618 us on one box:
  // the apply kernel indexes the by-value block per wave; sixteen workgroups' system-scope fences cost more than one
  // small kernel).  Taken out.)
#ifdef PPRHIP_TEST_HOOKS
  {  // PPRHIP_COUNT_LIVE=1 (measurement): share of a sweep's gathers that fetch a line with a non-zero, on stderr
    static const bool on = hook_env("PPRHIP_COUNT_LIVE") != nullptr;
    static unsigned long long* d_cnt = nullptr;
    static unsigned long long sweeps = 0;
    if (on && !backward) {
      if (!d_cnt) {
        PPRHIP_CHECK_HIP(hipMalloc((void**)&d_cnt, 16));
        PPRHIP_CHECK_HIP(hipMemset(d_cnt, 0, 16));
      }
      PPRHIP_TRY(launch_count_live_lines(P, d_cnt));
      if (++sweeps % 200 == 0) {
        unsigned long long h[2];
        PPRHIP_CHECK_HIP(hipMemcpy(h, d_cnt, 16, hipMemcpyDeviceToHost));
        fprintf(stderr, "[pprhip live lines] %llu sweeps: gathers of live lines %.3f of m, live lines %.3f of the sources, busy columns now %d\n",
                sweeps, (double)h[0] / (double)sweeps / (double)D->m, (double)h[1] / (double)sweeps / (double)D->n_src_live, n_active);
      }
    }
  }
#endif
  P->ktimer.begin(PPRHIP_KERNEL_DENSE_PULL_BATCH, sweep_bytes);
  PPRHIP_TRY(launch_dense_level_b8(P, backward, gs_blocks, n_gs));
  P->ktimer.end();
  bs->c8cur ^= 1;
  return fetch_begin(P, bs->sweep_out, sizeof(unsigned long long) * kBatch, &T->seq);
}

// true when the counters of a sweep in flight have arrived (collect_sweep would not wait)
bool sweep_arrived(const pprhip_graph* P, const SweepTicket& T) {
  return T.seq != 0 && P->mail && __atomic_load_n(&P->mail->seq, __ATOMIC_ACQUIRE) == T.seq;
}

int collect_sweep(pprhip_graph* P, ForaRun* runs, const SweepTicket& T) {
  PPRHIP_TRY(fetch_end(P, T.seq, P->batch->sweep_out, P->batch->h_sweep_out, sizeof(unsigned long long) * kBatch));
  for (int s = 0; s < kBatch; ++s)
    if (T.active[s]) {
      ForaRun& r = runs[T.ws[s]];
      const unsigned long long pk = P->batch->h_sweep_out[s];
      // the sweep's index stream is shared: each query is charged its own gathers and row work
      finish_dense(r.L, r.st, 8ull * P->gr->m + 36ull * T.rows + 4ull + 4ull * P->gr->m / (uint64_t)T.n_active,
                   batch_sweep_min_bytes(P, T.backward, T.n_active) / (uint64_t)T.n_active, (uint32_t)(pk >> kPackShift),
                   pk & kPackMask);
    }
  return PPRHIP_OK;
}

static int run_sweep(pprhip_graph* P, ForaRun* runs, const bool* active, int n_active) {
  SweepTicket T;
  PPRHIP_TRY(launch_sweep(P, runs, active, n_active, &T));
  return collect_sweep(P, runs, T);
}

// The vector, the selection and the per-query stats of a finished whole-graph FORA or top-k query (and of a query of the
// batched weighted FORA calls, weighted_batch.cpp)
int deliver_vector(BatchJob& J, ForaRun& r) {
  pprhip_graph* S = r.g;
  const int i = r.query;
  const bool topk = r.kind == QueryKind::kTopk;
  const double* vec = topk ? S->est : S->reserve;
  poll_idle(S);
  if (J.keep) {  // the vector stays in HBM after the slot moves on (internal order; pprhip_results_fetch permutes)
    {
      SetupScope setup(S);
      PPRHIP_TRY(launch_copy_f64(S, vec, J.keep->buf + (size_t)(J.keep_first + i) * J.P->gr->n, (size_t)J.P->gr->n));
    }
  }
  if (J.reserve_out) {
    double* dst = J.reserve_out + (size_t)i * J.P->gr->n;
    if (J.pipe) PPRHIP_TRY(J.pipe->submit(S, vec, dst));
    else PPRHIP_TRY(copy_out(S, vec, dst));
  }
  if (topk || J.k > 0) {  // (a top-k run's final selection wrote the first min(nsel, k) pairs of its block)
    int nsel = topk ? r.nsel : 0;
    bool have = false;
    int32_t* ids = topk ? r.ids_out : J.ids_out + (size_t)i * J.k;
    double* vals = topk ? r.vals_out : J.vals_out + (size_t)i * J.k;
    if (!topk) PPRHIP_TRY(select_topk(S, S->reserve, J.k, ids, vals, J.k, &nsel, nullptr, &have, r.st));
    for (int j = std::min(nsel, J.k); j < J.k; ++j) {
      ids[j] = -1;
      vals[j] = 0.0;
    }
    if (J.n_out) J.n_out[i] = nsel;
  }
  if (J.per_query) J.per_query[i] = r.st;
  return PPRHIP_OK;
}

// outputs of a finished query (its slot still holds the vectors)
int finish_query(BatchJob& J, ForaRun& r) {
  pprhip_graph* S = r.g;
  S->seed_on = false;  // (the query's pushes are over: a later query of the workspace must not land on its table)
  switch (r.kind) {
    case QueryKind::kFora:
    case QueryKind::kTopk:
    case QueryKind::kTargets: PPRHIP_TRY(deliver_vector(J, r)); break;
    case QueryKind::kPairs: {  // the values are in the call's device array; the phase times before the events are reused
      const hipEvent_t* ev = &r.pp->ev[3 * S->ws_index];
      PPRHIP_CHECK_HIP(hipEventSynchronize(ev[2]));
      r.st.push_ms = CallTimer::ms(ev[0], ev[1]);
      r.st.mc_ms = CallTimer::ms(ev[1], ev[2]);
      break;
    }
    case QueryKind::kBackward: break;  // (its triples join the job's below)
  }
  {
    std::lock_guard<std::mutex> lk(J.sum_mu);
    if (r.kind == QueryKind::kBackward) J.triples->insert(J.triples->end(), r.triples.begin(), r.triples.end());
    add_stats(J.sum, r.st);
  }
  r.triples.clear();
  r.phase = ForaRun::kDone;
  r.query = -1;
  return PPRHIP_OK;
}

// A query of a job of seed sets begins as pprhip_fora_seeds / pprhip_fora_topk_seeds begin theirs: its plan goes to the
// workspace's seed table, and the workspace lands dead-end mass on that table until finish_query.
int begin_query(BatchJob& J, ForaRun& r, pprhip_graph* S, int i) {
  S->tun = J.P->tun;
  S->seed_on = false;
  bool seeded = false;  // kFora and kTopk without sources: the query runs from seed set i
  const auto src = [&] { return J.P->gr->h_old2new[J.srcs[i]]; };  // internal id of source / target i
  switch (J.kind) {
    case QueryKind::kFora:
      seeded = !J.srcs;
      if (seeded) PPRHIP_TRY(fora_begin_seeds(r, S, J.sets[(size_t)i], J.eps, J.conf, J.seed, J.n_rounds));
      else PPRHIP_TRY(fora_begin(r, S, src(), J.eps, J.conf, J.seed, J.n_rounds));
      break;
    case QueryKind::kTopk: {
      seeded = !J.srcs;
      int32_t* const ids = J.ids_out + (size_t)i * J.k;
      double* const vals = J.vals_out + (size_t)i * J.k;
      const uint64_t seed = J.seed + (uint64_t)i;
      if (seeded) PPRHIP_TRY(topk_begin_seeds(r, S, J.sets[(size_t)i], J.eps, J.conf, seed, ids, vals, J.k));
      else PPRHIP_TRY(topk_begin(r, S, src(), J.eps, J.conf, seed, ids, vals, J.k));
      break;
    }
    case QueryKind::kBackward:
      pprhip_tuning_batch(&S->tun);  // level shapes only: a backward search has no cost-model decisions
      PPRHIP_TRY(bwd_begin(r, S, src(), J.srcs[i], J.alpha, J.threshold));
      break;
    case QueryKind::kPairs:  // the handle's tuning (include/pprhip.h "single pairs")
      PPRHIP_TRY(pair_begin(r, S, *J.pairs, src(), J.pairs->first[(size_t)i], J.pairs->first[(size_t)i + 1]));
      break;
    case QueryKind::kTargets:  // the handle's tuning (include/pprhip.h "single targets")
      PPRHIP_TRY(target_begin(r, S, *J.targets, i));
      break;
  }
  S->seed_on = seeded;
  r.query = i;
  r.job = &J;
  return PPRHIP_OK;
}

// Whole-graph FORA on one host thread: a query's walk phase goes to a side stream and runs beside the other queries'
// sweeps - with few waves per CU (the walks are bound by the memory system from four waves per CU on,
// tools/micro/chain_rate.hip), so that the compute stream's kernels find room beside it: 292 -> 327 queries/s on
// R-MAT 22 (16 waves per CU beside: 307; 2: 300).
static hipStream_t side_stream_for_walks(pprhip_graph* P) {
  BatchState* bs = P->batch;
  if (!bs->walk_stream_tried) {
    bs->walk_stream_tried = true;
    const char* e = hook_env("PPRHIP_BATCH_WALKS_BESIDE");
    if (!(e && e[0] == '0') && make_side_stream(P, &bs->walk_stream) != PPRHIP_OK) bs->walk_stream = nullptr;
  }
  if (bs->walk_stream)  // (every call: workspaces may have joined since)
    for (pprhip_graph* S : bs->slots)
      for (auto& ev : S->walk_ev)
        if (!ev && hipEventCreate(&ev) != hipSuccess) {
          ev = nullptr;
          (void)hipStreamDestroy(bs->walk_stream);
          bs->walk_stream = nullptr;
          return nullptr;
        }
  return bs->walk_stream;
}

// The stream the slots of the sequential driver work on: it has to run beside the compute stream (the sweeps) and
// beside the walk stream.  PPRHIP_BATCH_SLOTS_BESIDE=0: the slots stay on the compute stream (the driver of rounds 1-4).
static hipStream_t stream_for_slots(pprhip_graph* P) {
  BatchState* bs = P->batch;
  if (!bs->slot_stream_tried) {
    bs->slot_stream_tried = true;
    const char* e = hook_env("PPRHIP_BATCH_SLOTS_BESIDE");
    if (!(e && e[0] == '0')) {
      if (make_side_stream(P, &bs->slot_stream, bs->walk_stream) != PPRHIP_OK) bs->slot_stream = nullptr;
      if (!bs->slot_stream && bs->walk_stream && make_side_stream(P, &bs->slot_stream) != PPRHIP_OK) bs->slot_stream = nullptr;
    }
  }
  return bs->slot_stream;
}

// ------------------------------------------------------------------ the one-thread driver (batch_driver.hpp: SlotDriver)
// Where the walk phases and the workspaces run, then the workspaces themselves; the walk stream is resolved again for
// the events of the workspaces that joined in setup.  walks_beside: whole-graph FORA (the other kinds have no walk phase
// to put beside the sweeps).
int SlotDriver::open(pprhip_graph* P_, bool pool, bool walks_beside) {
  side = walks_beside ? side_stream_for_walks(P_) : nullptr;
  PPRHIP_TRY(setup(P_, pool, stream_for_slots(P_)));
  if (side) side = side_stream_for_walks(P_);  // (the new workspaces' events)
  return PPRHIP_OK;
}

// Cycles until after_cycle(busy) says kStop or anything fails.  No exception may cross the C ABI or leave a driver
// thread (it would end the process), and the driver's containers and callbacks allocate: the message is
// "<who>: <what><where>".
int SlotDriver::run(const char* who, const char* where, const std::function<int(int busy)>& after_cycle) {
  try {
    for (;;) {
      int busy = 0;
      PPRHIP_TRY(cycle(&busy));
      const int answer = after_cycle(busy);
      if (answer != kGoOn) return answer == kStop ? PPRHIP_OK : answer;
    }
  } catch (const std::exception& ex) {
    set_error("%s: %s%s", who, ex.what(), where);
    return PPRHIP_ERR_OOM;
  }
}

// pool: more workspaces than columns; slots_on: the stream the workspaces run on from here on (nullptr /
// P->stream: everything in stream order, as before round 5)
int SlotDriver::setup(pprhip_graph* P_, bool pool, hipStream_t slots_on) {
  P = P_;
  n_ws = kBatch;
  if (pool) {
    int want = kDefaultWs;
    if (const char* e = tuning_env("PPRHIP_BATCH_WORKSPACES")) want = std::max(kBatch, std::min(kMaxWs, atoi(e)));
    if (want > kBatch && ensure_workspaces(P, want) != PPRHIP_OK) {  // (no memory for them: one per column)
      (void)hipGetLastError();
      want = kBatch;
    }
    n_ws = want;
  }
  for (int c = 0; c < kBatch; ++c) P->batch->col_owner[c] = -1;
  for (size_t w = 0; w < P->batch->slots.size(); ++w) {
    pprhip_graph* S = P->batch->slots[w];
    S->stream = slots_on ? slots_on : P->stream;
    S->c8_via_parent = S->stream != P->stream;
    S->sync = nullptr;
    S->pooled = (int)w < n_ws;
    S->has_col = false;
  }
  // the workspaces' read-backs look after the sweep in flight while they wait (only worth it when they wait on
  // another stream than the sweep's)
  if (slots_on && slots_on != P->stream && !hook_env("PPRHIP_BATCH_NO_HOOK")) {
    P->batch->idle_hook = &SlotDriver::on_idle;
    P->batch->idle_arg = this;
  }
  return PPRHIP_OK;
}
void SlotDriver::teardown() {
  prof.print();
  P->batch->idle_hook = nullptr;
  P->batch->idle_arg = nullptr;
  if (P->batch->slot_stream) (void)hipStreamSynchronize(P->batch->slot_stream);
  for (size_t w = 0; w < P->batch->slots.size(); ++w) {  // (as the other drivers expect them)
    P->batch->slots[w]->pooled = P->batch->slots[w]->has_col = false;
    P->batch->slots[w]->slot_index = (int)(w % kBatch);
  }
}
void SlotDriver::on_idle(void* self) {
  SlotDriver* D = static_cast<SlotDriver*>(self);
  if (D->in_turn || D->hook_rc != PPRHIP_OK) return;
  if (D->flying) {
    if (!sweep_arrived(D->P, D->ticket)) return;
  } else {  // nothing on the compute stream (a call's first queries are still starting): whoever stands ready goes
    static const bool early = hook_env("PPRHIP_BATCH_NO_EARLY") == nullptr;
    if (!early) return;
    bool any = false;
    for (int w = 0; w < D->n_ws && !any; ++w) any = D->runs[w].query >= 0 && D->runs[w].waiting;
    if (!any) return;
  }
  D->prof.n[5]++;
  // (a turn taken from inside a workspace's wait may find that workspace's timer swapped in - a walk phase on the
  // side stream runs under a quiet one: the turn's own brackets belong to the timer the driver was started under)
  KernelTimer* const caller_timer = g_timer_cur;
  g_timer_cur = D->own_timer;
  const int rc = D->turn();
  g_timer_cur = caller_timer;
  if (rc != PPRHIP_OK) {
    D->hook_rc = rc;
    D->hook_msg = get_error();
  }
}

// a workspace that holds its column without standing at a dense level lets it go (its column is all-zero, or the
// compaction that makes it so is queued on the compute stream)
void SlotDriver::release_if_idle(int w) {
  pprhip_graph* S = P->batch->slots[w];
  if (S->has_col && !(runs[w].query >= 0 && runs[w].waiting)) {
    P->batch->col_owner[S->slot_index] = -1;
    S->has_col = false;
  }
}

// one workspace as far as it gets: until it waits at a dense level, for its column or for its walk phase, or there is
// nothing to start.  defer: it must not wait for the device (the next sweep is not launched yet).
int SlotDriver::step_ws(int w, bool defer) {
  ForaRun& r = runs[w];
  int rc = PPRHIP_OK;
  const int outer = cur_ws;
  if (!defer) {
    cur_ws = w;
    col_marked[w] = false;
  }
  for (;;) {
    if (r.query < 0) {
      if (defer) break;
      BatchJob* J = nullptr;
      int i = -1;
      if (!next(&J, &i)) break;
      if ((rc = begin_query(*J, r, P->batch->slots[w], i)) != PPRHIP_OK) break;
      r.side = side;
    }
    if (r.waiting) break;
    if (defer) {
      // only a run that stands between two levels of a push can answer without the device: a frontier it can
      // sweep (again), or one that goes back to list form (the compaction is queued; the levels follow later)
      const bool in_levels =
          r.phase == ForaRun::kLevels || r.phase == ForaRun::kTopkLevels || r.phase == ForaRun::kBwdLevels;
      if (!in_levels || r.L.nf == 0 || r.L.compacted) break;
      if (!r.L.dense_prepared) {  // (a run that stood waiting for its column: its next level is a dense one)
        bool dense = false;
        (void)level_cost(r.g, r.L.nf, r.L.ef, &dense);
        if (!dense) break;
      }
      r.L.defer_compact = true;
    }
    P->batch->slots[w]->c8_settled = defer;
    rc = run_step(r, true);
    P->batch->slots[w]->c8_settled = false;
    r.L.defer_compact = false;
    if (rc != kYieldColumn) col_marked[w] = false;  // (it no longer stands ready for a column)
    if (rc == kYield) {
      r.waiting = true;
      rc = PPRHIP_OK;
      break;
    }
    if (rc == kYieldColumn && !defer) {
      // what it has queued so far must have ended before it may take the column without waiting for the stream
      pprhip_graph* S = P->batch->slots[w];
      if (!S->col_ev && hipEventCreateWithFlags(&S->col_ev, hipEventDisableTiming) != hipSuccess) S->col_ev = nullptr;
      col_marked[w] = S->col_ev && hipEventRecord(S->col_ev, S->stream) == hipSuccess;
    }
    if (rc == kYieldDefer || rc == kYieldColumn) {
      rc = PPRHIP_OK;
      break;
    }
    if (rc == kYieldWalk) {
      walking[w] = true;
      rc = PPRHIP_OK;
      break;
    }
    if (rc != PPRHIP_OK) break;
    BatchJob* const J = r.job;
    if ((rc = finish_query(*J, r)) != PPRHIP_OK) break;
    done(J);
  }
  if (!defer) cur_ws = outer;
  release_if_idle(w);
  if (rc == PPRHIP_OK && hook_rc != PPRHIP_OK) {
    set_error("%s", hook_msg.c_str());
    rc = hook_rc;
  }
  return rc;
}

// collect the sweep in flight, let its queries (and the ones that stand ready for the columns let go) say what they do
// next, launch the next sweep: nothing in here waits for the device beyond the sweep's counters
int SlotDriver::turn() {
  in_turn = true;
  const int rc = turn_body();
  in_turn = false;
  return rc;
}
int SlotDriver::turn_body() {
  prof.start();
  if (flying) {
    PPRHIP_TRY(collect_sweep(P, runs, ticket));
    flying = false;
    prof.lap(0);
    for (int c = 0; c < kBatch; ++c)
      if (ticket.active[c]) {
        const int w = ticket.ws[c];
        runs[w].waiting = false;
        PPRHIP_TRY(step_ws(w, true));
        prof.lap(runs[w].waiting ? 1 : 2);
      }
    // columns have been let go: workspaces that stand ready prepare their levels behind the compactions
    int n_free = 0;
    for (int c = 0; c < kBatch; ++c) n_free += P->batch->col_owner[c] < 0 ? 1 : 0;
    for (int t = 0; t < n_ws && n_free > 0; ++t) {
      const int w = (ready_rr + t) % n_ws;
      if (w == cur_ws || runs[w].query < 0 || walking[w] || runs[w].waiting || !col_marked[w] ||
          hipEventQuery(P->batch->slots[w]->col_ev) != hipSuccess)
        continue;
      PPRHIP_TRY(step_ws(w, true));
      prof.lap(3);
      if (runs[w].waiting) {
        n_free--;
        ready_rr = (w + 1) % n_ws;
      }
    }
  }
  // (Tried for the end of a call, round 5: with nothing left to start and at most 2 / 3 / 4 queries still in their
  // push, those queries took their column of c8 into vectors of their own and finished with the single-query level
  // kernels - 0.36 ms per level each against 1.6 ms per sweep for any number of columns.  Parity-green and without
  // effect: 350-353 against 351-354 queries/s, the same 857-859 sweeps - a call's last sweeps run at 4-12 busy
  // columns for most of the drain and at <= 4 only for its last few levels.  Taken out.)
  bool active[kBatch];
  int ws[kBatch];
  int n_wait = 0;
  for (int c = 0; c < kBatch; ++c) {
    const int w = P->batch->col_owner[c];
    active[c] = w >= 0 && runs[w].query >= 0 && runs[w].waiting;
    ws[c] = active[c] ? w : c;
    n_wait += active[c] ? 1 : 0;
  }
  if (n_wait) {
    prof.start();
    PPRHIP_TRY(launch_sweep(P, runs, active, n_wait, &ticket, ws));
    flying = true;
    prof.lap(4);
  }
  return PPRHIP_OK;
}

// One cycle (batch_driver.hpp: SlotDriver).  *busy: the workspaces that hold a query afterwards; with none and nothing to start the
// caller is done (or waits for work).
// (The pass over the other workspaces takes them through their steps one after the other, each step waiting for its
// own read-backs.  Tried, round 5: batches of sparse levels launched and collected separately - run_levels returned
// behind the launches and was called again when the mailbox had the counters, so that all workspaces' first levels
// were in flight together, with the first sweep of a call held until the others stood ready.  Parity-green and no
// faster: R-MAT 22 355-356 against 358-359 queries/s, R-MAT 20 1 175 against 1 194, 50 per call 310.7 against 311.8 -
// a call's length is set by the chain of sweeps each column's queries need, not by how fast the first ones start.
// Taken out.)
int SlotDriver::cycle(int* busy) {
  PPRHIP_TRY(turn());
  // the workspaces that are not in the sweep
  const int first = rr;
  for (int t = 0; t < n_ws; ++t) {
    const int w = (first + t) % n_ws;
    if (runs[w].query >= 0 && runs[w].waiting) continue;  // in the sweep
    if (flying && sweep_arrived(P, ticket)) {  // the compute stream is idle: the sweep's queries come first
      rr = w;
      break;
    }
    if (walking[w]) {
      if (hipEventQuery(P->batch->slots[w]->walk_ev[2]) == hipErrorNotReady) continue;
      walking[w] = false;
    }
    if (col_marked[w]) {  // it stands ready for a column: nothing to do for it while none is free
      bool any_free = false;
      for (int c = 0; c < kBatch && !any_free; ++c) any_free = P->batch->col_owner[c] < 0;
      if (!any_free) continue;
    }
    PPRHIP_TRY(step_ws(w, false));
  }
  *busy = 0;
  int n_wait = 0, n_pending = 0, first_walk = -1;
  for (int w = 0; w < n_ws; ++w) {
    const bool has = runs[w].query >= 0;
    *busy += has ? 1 : 0;
    n_wait += (has && runs[w].waiting) ? 1 : 0;
    // (left behind by a turn taken from inside this pass, after the pass had gone by: the next cycle takes it on)
    n_pending += (has && !runs[w].waiting && !walking[w]) ? 1 : 0;
    if (walking[w] && first_walk < 0) first_walk = w;
  }
  if (*busy > 0 && !flying && n_wait == 0 && n_pending == 0) {
    // nobody stands at a dense level and no sweep is on its way: a walk phase has to end before anything can go on
    if (first_walk < 0) {
      set_error("batch driver: %d queries in flight, none waiting", *busy);
      return PPRHIP_ERR_STATE;
    }
    PPRHIP_CHECK_HIP(hipEventSynchronize(P->batch->slots[first_walk]->walk_ev[2]));
  }
  return PPRHIP_OK;
}
// Queries left over when a call's count is not a multiple of the slots: up to kTailSingle of them run one at a time on
// the handle's own workspace (the single-query path: 10 ms each on R-MAT 22) instead of as a last round of sweeps with
// nearly all columns empty - a sweep costs the same for 2 busy columns as for 16, so such a round takes most of a
// query's latency.  PPR.java:179's 50 queries per call = 3 x 16 + 2: 178 -> 172 ms per call.
constexpr int kTailSingle = 3;
static int tail_queries(const BatchJob& J) {
  return (is_whole_graph(J.kind) && J.q > kBatch && J.q % kBatch <= kTailSingle && !hook_env("PPRHIP_BATCH_NO_TAIL")) ? J.q % kBatch : 0;
}
static int run_tail(BatchJob& J, int q_slots) {
  for (int i = q_slots; i < J.q; ++i) {  // the stragglers, one at a time on the handle's own vectors
    ForaRun r;
    int rc = begin_query(J, r, J.P, i);  // (a seed set: the single-query seeded path, on the handle's own table)
    if (rc == PPRHIP_OK) {
      r.side = nullptr;
      while ((rc = run_step(r, false)) == kYield) {
      }
    }
    if (rc == PPRHIP_OK) rc = finish_query(J, r);
    if (rc != PPRHIP_OK) {
      J.P->seed_on = false;
      return rc;
    }
  }
  return PPRHIP_OK;
}

// The queries of a whole-graph FORA call (one seed, stream 0) draw the same walks: from kWalkShareMinQueries queries on
// they share terminals through the batch state's cache (engine.hpp: WalkShare).  Called with no walk kernel of the
// slots in flight: before a call's first query, or by a stream's driver that stands idle.
void share_walks_of(BatchJob& J) {
  pprhip_graph* P = J.P;
  double rmax = 0.0, omega = 0.0;
  if (!is_whole_graph(J.kind) || fora_start_params(P->batch->slots[0], J.eps, J.conf, J.n_rounds, &rmax, &omega) != PPRHIP_OK) {
    if (P->batch->share) P->batch->share->on = false;
    return;
  }
  walk_share_begin(P, J.q, J.conf->alpha, rmax, omega, J.seed);
}

// all queries on the calling thread (SlotDriver)
static int batch_sequential(BatchJob& J) {
  pprhip_graph* P = J.P;
  std::unique_ptr<SlotDriver> Dp(new (std::nothrow) SlotDriver());
  if (!Dp) return PPRHIP_ERR_OOM;
  SlotDriver& D = *Dp;
  PPRHIP_TRY(D.open(P, is_whole_graph(J.kind) && J.q > kBatch, is_whole_graph(J.kind)));
  KernelTimer& tm = ktimer();  // (the call's timer watches the stream the workspaces' kernels run on ...)
  tm.stream = P->batch->slots[0]->stream;
  // queries the workspaces run (the leftover rule is for one workspace per column: with the pool there are no rounds
  // of 16 whose last one would be nearly empty - 50 / 51 / 35 sources per call: 306 / 302 / 281 queries/s without
  // the rule, 306 / 292 / 270 with it).
  // (A query is a chain of ~26 dense levels and a column serves one level per sweep: 50 queries on 16 columns cost two
  // columns four queries' worth of sweeps, ~104, whatever the order.  Tried against that, round 5: the q mod 16 <= 4
  // leftovers on a helper thread and a stream of their own BESIDE the batch, each on a workspace that runs
  // single-query dense levels over vectors of its own, so that the other 48 take three queries' worth.  Parity-green
  // and no faster - 50 / 51 / 35 / 20 sources per call: 314 / 304 / 281 / 225 queries/s against 310 / 306 / 285 / 252: the
  // single-query edge kernel (a 1024-thread workgroup with a 128-KB table per CU) does not fit on a CU beside the
  // batched one, so its levels run in the gaps between the sweeps' kernels, one per sweep period - as in a column.
  // Taken out; the query stream is the answer for calls that follow one another: 351-362 queries/s on blocks of 50.)
  const int q_slots = J.q - (D.n_ws > kBatch ? 0 : tail_queries(J));
  D.next = [&](BatchJob** job, int* i) {
    *i = J.next_query.fetch_add(1);
    *job = &J;
    return *i < q_slots;
  };
  D.done = [](BatchJob*) {};
  const int rc = D.run("batch driver", "", [](int busy) { return busy == 0 ? SlotDriver::kStop : SlotDriver::kGoOn; });
  D.teardown();
  if (rc != PPRHIP_OK) return rc;
  if (tm.stream != P->stream) {  // (... and the stragglers' on the handle's own)
    (void)hipStreamSynchronize(P->stream);
    tm.fold();
    tm.stream = P->stream;
  }
  return run_tail(J, q_slots);
}

// (Round 4 also ran this driver on 2 - 16 host threads that shared the one compute stream, the slots dealt out between
// them and the threads meeting once per sweep - the idea being that the transitions of different threads' slots fill
// each other's gaps in the stream, which idles 12-18 % of the time behind the host's decisions.  It got slower with
// every thread added: 326 / 322 / 315 / 307 / 301 queries/s with 1 / 2 / 4 / 8 / 16 threads, the sweeps themselves
// 1 334 -> 1 443 us (profiles/r04_driver_threads_study.txt) - several threads launching into one stream pay more in the
// runtime than the gaps they close.  Taken out.  Round 5 closes the gaps from ONE thread instead: SlotDriver.)

// one worker thread per slot
static void batch_worker(BatchJob* J, BatchSync* B, ForaRun* runs, int s) {
  pprhip_graph* P = J->P;
  pprhip_graph* S = P->batch->slots[s];
  ForaRun& r = runs[s];
  int rc = PPRHIP_OK;
  if (hipSetDevice(P->gr->device) != hipSuccess) {
    set_error("hipSetDevice(%d) failed in a batch worker", P->gr->device);
    rc = PPRHIP_ERR_HIP;
  }
  KernelTimer* const own_timer = g_timer_cur;
  g_timer_cur = &S->ktimer;
  S->ktimer.stream = S->stream;
  S->ktimer.reset();
  while (rc == PPRHIP_OK) {
    {
      std::lock_guard<std::mutex> lk(B->mu);
      if (B->err) break;
    }
    const int i = J->next_query.fetch_add(1);
    if (i >= J->q) break;
    rc = begin_query(*J, r, S, i);
    while (rc == PPRHIP_OK) {
      rc = run_step(r, true);
      if (rc != kYield) break;
      rc = B->arrive(s);
    }
    if (rc == PPRHIP_OK) rc = finish_query(*J, r);
  }
  if (rc != PPRHIP_OK) {
    leave_push(r);
    S->seed_on = false;
    B->fail(rc);
  }
  (void)hipStreamSynchronize(S->stream);
  g_timer_cur = own_timer;
  B->worker_done(s);
}

}  // namespace detail

// ------------------------------------------------------------------ the threaded driver's rendezvous (engine_internal.hpp)
void BatchSync::release(int s) {
  std::lock_guard<std::mutex> lk(mu);
  if (hold[s]) {
    hold[s] = false;
    n_hold--;
    cv.notify_all();
  }
}

void BatchSync::c8_enter(int s) {
  std::unique_lock<std::mutex> lk(mu);
  cv.wait(lk, [&] { return !sweeping || err != 0; });
  if (!hold[s]) {
    hold[s] = true;
    n_hold++;
  }
}

void BatchSync::fail(int rc) {
  std::lock_guard<std::mutex> lk(mu);
  if (!err) {
    err = rc;
    errmsg = get_error();
  }
  cv.notify_all();
}

void BatchSync::worker_done(int s) {
  std::lock_guard<std::mutex> lk(mu);
  if (hold[s]) {
    hold[s] = false;
    n_hold--;
  }
  n_workers--;
  cv.notify_all();
}

int BatchSync::arrive(int s) {
  std::unique_lock<std::mutex> lk(mu);
  if (err) return err;
  if (hold[s]) {
    hold[s] = false;
    n_hold--;
  }
  waitflag[s] = true;
  n_wait++;
  cv.notify_all();
  cv.wait(lk, [&] { return !waitflag[s] || err != 0; });
  return err;
}

// the sweeper thread: one batched sweep whenever somebody waits and nobody holds
void BatchSync::sweeper() {
  (void)hipSetDevice(P->gr->device);
  std::unique_lock<std::mutex> lk(mu);
  for (;;) {
    cv.wait(lk, [&] { return n_workers == 0 || err != 0 || (n_wait > 0 && n_hold == 0); });
    if (n_workers == 0 || err != 0) return;
    sweeping = true;
    bool active[kBatch];
    int n_active = 0;
    for (int s = 0; s < kBatch; ++s) {
      active[s] = waitflag[s];
      n_active += active[s] ? 1 : 0;
    }
    lk.unlock();
    const int rc = run_sweep(P, runs, active, n_active);
    const std::string msg = rc != PPRHIP_OK ? get_error() : "";
    lk.lock();
    if (rc != PPRHIP_OK && !err) {
      err = rc;
      errmsg = msg;
    }
    for (int s = 0; s < kBatch; ++s)
      if (active[s]) {
        waitflag[s] = false;
        n_wait--;
        hold[s] = true;  // until the slot has said what it does next
        n_hold++;
      }
    sweeping = false;
    cv.notify_all();
  }
}

}  // namespace pprhip

// runs a prepared job on the handle's slots (both batched entry points)
#ifdef PPRHIP_TEST_HOOKS
// PPRHIP_APPLY_COUNT_RES=1 (hooks library): what the batched apply counted on dead-end tiles since the last look, in the
// unused class 7 of a call's statistics - class_bytes: the non-zero residues it met (it takes them for zero without the
// switch: DESIGN.md §5), class_launches: the residues it loaded to see, class_ms: the dead-end tiles an entry sweep came
// by.  On the sweeps' stream, behind the sweeps launched so far.
int pprhip::detail::take_apply_counts(pprhip_graph* g, pprhip_stats_t& sum) {
  if (!hook_env("PPRHIP_APPLY_COUNT_RES") || !g->batch || !g->batch->apply_res_count) return PPRHIP_OK;
  unsigned long long c[3] = {0, 0, 0};
  PPRHIP_CHECK_HIP(hipMemcpyAsync(c, g->batch->apply_res_count, sizeof c, hipMemcpyDeviceToHost, g->stream));
  PPRHIP_CHECK_HIP(hipMemsetAsync(g->batch->apply_res_count, 0, sizeof c, g->stream));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  sum.class_bytes[7] = c[0];
  sum.class_launches[7] = (uint32_t)std::min<unsigned long long>(c[1], 0xffffffffull);
  sum.class_ms[7] = (double)c[2];
  return PPRHIP_OK;
}
#endif

int pprhip::detail::batch_run(pprhip_graph_t* g, BatchJob& J, pprhip_stats_t* stats_sum) {
  PPRHIP_TRY(ensure_batch(g));
  if (pushes_backward(J.kind)) PPRHIP_TRY(ensure_bwd_layout(g));
  const int q = J.q;
  // Worker threads pay off where queries are latency-bound (top-k: short rounds of sparse levels, walks
  // and selections, 2.4x on R-MAT 22); whole-graph FORA keeps the memory system busy from one thread.
  const char* env = tuning_env("PPRHIP_BATCH_THREADS");
  const bool threaded = q > 1 && (env ? env[0] == '1' : !is_whole_graph(J.kind));
  std::memset(&J.sum, 0, sizeof J.sum);
  // vectors go to the caller's memory behind the queries' backs (a synchronous copy of 8n bytes to pageable memory per
  // query would stall the one stream everything runs on: 170 instead of 270 queries/s on R-MAT 22)
  if (J.reserve_out && J.kind != QueryKind::kBackward && q > 1) {
    if (!g->batch->fetch) g->batch->fetch = new (std::nothrow) FetchPipe();
    if (!g->batch->fetch) return PPRHIP_ERR_OOM;
    const int prc = g->batch->fetch->ensure(g);
    if (prc != PPRHIP_OK) {
      g->batch->fetch->destroy();
      delete g->batch->fetch;
      g->batch->fetch = nullptr;
      return prc;
    }
    g->batch->fetch->start();
    J.pipe = g->batch->fetch;
  }
  ForaRun runs[kBatch];
  g->ktimer.stream = g->stream;
  g->ktimer.reset();
  const auto t0 = std::chrono::steady_clock::now();
  share_walks_of(J);
  int rc = PPRHIP_OK;
  double tot[8] = {0};
  uint64_t bytes[8] = {0};
  uint32_t cnt[8] = {0};
  if (threaded) {
    BatchSync B;
    B.P = g;
    B.runs = runs;
    for (pprhip_graph* S : g->batch->slots) {
      S->stream = S->own_stream;
      S->c8_via_parent = false;
      S->sync = &B;
    }
    B.n_workers = kBatch;
    std::thread sweeper(&BatchSync::sweeper, &B);
    std::vector<std::thread> workers;
    for (int s = 0; s < kBatch; ++s) workers.emplace_back(batch_worker, &J, &B, runs, s);
    for (auto& w : workers) w.join();
    sweeper.join();
    for (pprhip_graph* S : g->batch->slots) {
      S->sync = nullptr;
      S->ktimer.resolve(tot, bytes, cnt);
    }
    if (B.err) {
      set_error("%s", B.errmsg.c_str());
      rc = B.err;
    }
  } else {
    for (pprhip_graph* S : g->batch->slots) {
      S->stream = g->stream;
      S->c8_via_parent = false;
      S->sync = nullptr;
    }
    KernelTimer local;  // the caller's timer may be in use (All-Pair times its own tiers)
    KernelTimer* const saved = g_timer_cur;
    g_timer_cur = &local;
    local.stream = g->stream;
    rc = batch_sequential(J);
    (void)hipStreamSynchronize(g->stream);
    local.resolve(tot, bytes, cnt);
    local.destroy();
    g_timer_cur = saved;
  }
  (void)hipStreamSynchronize(g->stream);
  if (g->batch->share) g->batch->share->on = false;  // (the cache lives for one call)
  if (J.pipe) {
    const std::string msg = rc != PPRHIP_OK ? get_error() : std::string();
    const int prc = J.pipe->finish();  // every vector submitted so far has reached its destination
    J.pipe = nullptr;
    if (rc != PPRHIP_OK) set_error("%s", msg.c_str());
    else rc = prc;
  }
  if (rc != PPRHIP_OK) {
    const std::string msg = get_error();
    g->seed_on = false;  // (the leftover rule runs seed sets on the handle's own workspace)
    free_batch(g);  // slots may hold half-pushed levels (and seed tables): the next batched call builds clean ones
    set_error("%s", msg.c_str());
    return rc;
  }
  g->ktimer.resolve(tot, bytes, cnt);
  pprhip_stats_t& sum = J.sum;
  sum.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fold_class_totals(sum, tot, bytes, cnt);
#ifdef PPRHIP_TEST_HOOKS
  PPRHIP_TRY(take_apply_counts(g, sum));
#endif
  if (stats_sum) *stats_sum = sum;
  return PPRHIP_OK;
}
