// fora.cpp — FORA and FORA top-k as resumable runs (run.hpp), and the single-query entry points that drive them.  The
// runs that push backward are in bwd_runs.cpp, the batched entry points that keep kBatch runs in flight in batch.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "run.hpp"

using namespace pprhip;
using namespace pprhip::detail;

// ------------------------------------------------------------------ FORA whole graph (a5)
namespace pprhip {
namespace detail {

constexpr uint32_t kSideWalkWavesDefault = 4;  // waves per CU of a walk phase that runs beside sweeps (batch_sequential)
static uint32_t side_walk_waves() {  // PPRHIP_SIDE_WALK_WAVES: measurement switch
  static const uint32_t v = [] {
    const char* e = hook_env("PPRHIP_SIDE_WALK_WAVES");
    const long x = e ? atol(e) : 0;
    return x > 0 && x <= 32 ? (uint32_t)x : kSideWalkWavesDefault;
  }();
  return v;
}

void leave_push(ForaRun& r) {
  if (r.in_push) {
    r.in_push = false;
    if (r.g->sync) r.g->sync->release(r.g->slot_index);
  }
}

// omega and the threshold a whole-graph FORA query's first push runs at (every later one runs at a lower one)
int fora_start_params(const pprhip_graph* g, double eps, const pprhip_fora_conf_t* conf, int n_rounds, double* rmax_out,
                      double* omega_out) {
  double rmax = 0.0, omega = 0.0;
  PPRHIP_TRY(pprhip_fora_whole_params(conf, eps, &rmax, &omega));  // Fora_Whole_Graph.java:86-87
  if (n_rounds == 0 && g->tun.prior_levels > 0 && g->tun.halving_ratio > 1.0) {
    // Loop turns that are known to pass before any push: after a push at rmax every r(v) < rmax * d(v), so
    // rsum <= rmax * m and the walks cost at most c_walk * omega * (1 - alpha) * rmax * m; while that bound still
    // covers prior_levels dense levels the turn would be repeated at half the threshold anyway (twin: same rule).
    const pprhip_tuning_t& t = g->tun;
    double walk_bound = t.c_walk_ns * omega * (1 - conf->alpha) * rmax * (double)g->gr->m;
    const double push_est =
        (double)t.prior_levels * (t.c_level_ns + t.c_dense_edge_ns * (double)g->gr->m + t.c_dense_node_ns * (double)g->gr->n);
    for (int h = 0; h < t.max_halvings && walk_bound >= push_est; ++h) {
      walk_bound /= 2.0;
      rmax /= 2.0;
    }
  }
  *rmax_out = rmax;
  *omega_out = omega;
  return PPRHIP_OK;
}

// src_internal -1: the query runs from the seed table (g->seeds), whose largest id bounds the reset (reset_node)
static int fora_begin_at(ForaRun& r, pprhip_graph* g, int32_t src_internal, int32_t reset_node, double eps,
                         const pprhip_fora_conf_t* conf, uint64_t seed, int n_rounds) {
  r.g = g;
  r.kind = QueryKind::kFora;
  r.src = src_internal;
  r.seeded = src_internal < 0;
  r.conf = conf;
  r.seed = seed;
  r.n_rounds = n_rounds;
  std::memset(&r.st, 0, sizeof r.st);
  g->topk_active = false;
  PPRHIP_TRY(reset_query_state(g, false, reset_node));
  r.alpha = conf->alpha;
  r.rsum_local = conf->rsum;
  PPRHIP_TRY(fora_start_params(g, eps, conf, n_rounds, &r.rmax_local, &r.omega_local));
  r.rmax_used = r.rmax_local;
  r.model_cost = 0.0;
  r.rounds = 0;
  r.dead_src = !r.seeded && hdeg_out(g, src_internal) == 0;
  r.L = LevelCtx();
  r.phase = ForaRun::kRoundStart;
  r.waiting = false;
  r.in_push = true;
  return PPRHIP_OK;
}

int fora_begin(ForaRun& r, pprhip_graph* g, int32_t src_internal, double eps, const pprhip_fora_conf_t* conf,
               uint64_t seed, int n_rounds) {
  return fora_begin_at(r, g, src_internal, src_internal, eps, conf, seed, n_rounds);
}

// the same query from a seed set: the table is installed here, the push starts from it in round 0 (seed_start)
int fora_begin_seeds(ForaRun& r, pprhip_graph* g, SeedTable& plan, double eps, const pprhip_fora_conf_t* conf,
                     uint64_t seed, int n_rounds) {
  PPRHIP_TRY(fora_begin_at(r, g, -1, plan.max_id, eps, conf, seed, n_rounds));
  return seed_upload(g, plan);
}

int fora_step(ForaRun& r, bool yield_dense) {
  pprhip_graph* g = r.g;
  for (;;) {
    if (r.phase == ForaRun::kRoundStart) {  // Fora_Whole_Graph.java:93-103, clock replaced by the level cost model
      const bool more = r.n_rounds > 0 ? r.rounds < r.n_rounds
                                       : (r.model_cost < g->tun.c_walk_ns * r.rsum_local * r.omega_local &&
                                          r.rounds < g->tun.max_rounds);
      if (!more) {
        r.phase = ForaRun::kWalks;
        continue;
      }
      if (r.dead_src) {  // Forward_Push.java:72-76
        PPRHIP_TRY(launch_set_f64(g, g->reserve, (uint32_t)r.src, 1.0));
        r.rsum_local = 0.0;
        r.rmax_used = r.rmax_local;
        r.rounds++;
        r.phase = ForaRun::kWalks;
        continue;
      }
      r.a = PushArgs{r.alpha, r.rmax_local, 0.0, r.seeded ? -1 : r.src, kFwdWhole};
      r.cut = RoundCut();
      r.cut.fixed = r.n_rounds > 0;
      r.cut.enabled = r.n_rounds > 0 ? r.rounds + 1 < r.n_rounds : r.rounds + 1 < g->tun.max_rounds;
      r.cut.omega = r.omega_local;
      r.cut.c_walk = g->tun.c_walk_ns;
      r.cut.alpha = r.alpha;
      if (r.rounds == 0 && r.seeded) {
        PPRHIP_TRY(seed_start(g, r.L));
      } else if (r.rounds == 0) {
        PPRHIP_TRY(launch_set_f64(g, g->residue, (uint32_t)r.src, 1.0));
        PPRHIP_TRY(seed_single(g, r.L, r.src, hdeg_out(g, r.src)));
      } else {
        PPRHIP_TRY(seed_scan(g, r.a, 0, r.L));
      }
      r.phase = ForaRun::kLevels;
    }
    if (r.phase == ForaRun::kLevels) {
      const int rc = run_levels(g, r.a, r.L, r.st, &r.model_cost, yield_dense, &r.cut);
      if (rc != PPRHIP_OK) return rc;  // kYield or an error
      if (r.cut.taken && !r.cut.fixed) {
        r.rsum_local = r.cut.rsum;  // measured when the round was cut; nothing was pushed since
      } else {
        double sum = 0.0;
        PPRHIP_TRY(device_sum(g, g->residue, &sum));
        r.rsum_local = sum * (1 - r.alpha);  // :101 (rsum is the exact residue sum here)
      }
      r.rmax_used = r.rmax_local;
      r.rmax_local /= 2.0;  // :102
      // The reference's loop would turn again (and restart the push from scratch at half the threshold) as
      // long as the push stays cheaper than the walks; when the walks outweigh the push so far by ratio^k, k
      // further halvings are taken at once instead of pushing at every threshold between (the twin does the same).
      if (r.n_rounds == 0 && r.model_cost > 0.0 && g->tun.halving_ratio > 1.0) {
        double ratio = g->tun.c_walk_ns * r.rsum_local * r.omega_local / r.model_cost;
        for (int h = 1; ratio >= g->tun.halving_ratio && h < g->tun.max_halvings; ++h) {
          ratio /= g->tun.halving_ratio;
          r.rmax_local /= 2.0;
        }
      }
      r.rounds++;
      r.phase = (r.n_rounds > 0 && !(r.rsum_local > 0.0)) ? ForaRun::kWalks : ForaRun::kRoundStart;
      continue;
    }
    if (r.phase == ForaRun::kWalks) {
      leave_push(r);
      if (r.tm) r.tm->mark(1);
      // Fora_Whole_Graph.java:112-140
      const double nrw_d = r.omega_local * r.rsum_local;
      const long long nrw = (nrw_d == nrw_d && nrw_d > 0.0) ? (long long)nrw_d : 0;
      if (!r.dead_src && r.side) {
        // the walk phase beside the other queries' sweeps: plan and walks on the side stream, behind everything this
        // query has queued on the compute stream; the driver calls again when walk_ev[2] has passed
        PPRHIP_CHECK_HIP(hipEventRecord(g->walk_ev[0], g->stream));
        PPRHIP_CHECK_HIP(hipStreamWaitEvent(r.side, g->walk_ev[0], 0));
        hipStream_t own = g->stream;
        KernelTimer* const tsave = g_timer_cur;
        KernelTimer quiet;
        quiet.off = true;  // (timed by the events below: the caller's timer watches the compute stream)
        g_timer_cur = &quiet;
        g->stream = r.side;
        g->walk_waves = side_walk_waves();
        int rc = hipEventRecord(g->walk_ev[1], r.side) == hipSuccess ? PPRHIP_OK : PPRHIP_ERR_HIP;
        if (rc == PPRHIP_OK) rc = run_walk_phase(g, 0, r.alpha, r.rsum_local, nrw, r.seed, 0, g->reserve, r.st);
        if (rc == PPRHIP_OK && hipEventRecord(g->walk_ev[2], r.side) != hipSuccess) rc = PPRHIP_ERR_HIP;
        g->stream = own;
        g->walk_waves = 0;
        g_timer_cur = tsave;
        PPRHIP_TRY(rc);
        r.phase = ForaRun::kWalkWait;
        return kYieldWalk;
      }
      if (!r.dead_src) {
        // (a worker's walks run beside the other slots' sweeps as well: the same narrow grid as on the side stream)
        if (g->sync && !hook_env("PPRHIP_WORKER_WALK_WIDE")) g->walk_waves = side_walk_waves();
        const int rc = run_walk_phase(g, 0, r.alpha, r.rsum_local, nrw, r.seed, 0, g->reserve, r.st);
        g->walk_waves = 0;
        PPRHIP_TRY(rc);
      }
      r.phase = ForaRun::kWalkWait;
    }
    if (r.phase == ForaRun::kWalkWait) {
      if (!r.dead_src && r.side) {
        PPRHIP_CHECK_HIP(hipEventSynchronize(g->walk_ev[2]));  // (the driver has seen it pass)
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g->walk_ev[1], g->walk_ev[2]) == hipSuccess) {
          ktimer().acc_ms[PPRHIP_KERNEL_WALK] += (double)ms;  // plan + walks, as one launch of the class
          ktimer().acc_cnt[PPRHIP_KERNEL_WALK]++;
        }
      }
      if (r.tm) r.tm->mark(2);
      PPRHIP_TRY(read_dead_pops(g, r.st));  // one read-back for the push's dead-end pops and the walks' steps
      r.st.rounds = (uint32_t)r.rounds;
      r.st.rsum = r.rsum_local;
      r.st.rmax_final = r.rmax_used;
      r.st.omega = r.omega_local;
      r.phase = ForaRun::kDone;
    }
    return PPRHIP_OK;
  }
}

// Fora_Topk.computeTopKPPR (Fora_Topk.java:102-184) as a resumable run: the one loop of every top-k entry point
// (pprhip_fora_topk, pprhip_fora_topk_seeds, the batched calls and streams).  src_internal -1: from the seed table
// (plan), whose largest id bounds the reset.
static int topk_begin_at(ForaRun& r, pprhip_graph* g, int32_t src_internal, SeedTable* plan, double eps,
                         const pprhip_fora_conf_t* conf, uint64_t seed, int32_t* ids_out, double* vals_out, int cap) {
  r = ForaRun();  // (every field of the loop at its start value)
  r.g = g;
  r.kind = QueryKind::kTopk;
  r.src = src_internal;
  r.seeded = plan != nullptr;
  r.conf = conf;
  r.seed = seed;
  PPRHIP_TRY(topk_session_reset(g, src_internal, plan, conf->alpha, conf->rsum));
  r.alpha = conf->alpha;
  r.sched = TopkSchedule(eps * 0.5, conf);  // :109-110, :113
  r.delta_local = conf->delta;
  r.rsum_local = conf->rsum;
  r.ids_out = ids_out;
  r.vals_out = vals_out;
  r.cap = cap;
  r.phase = ForaRun::kTopkRoundStart;
  return PPRHIP_OK;
}

int topk_begin(ForaRun& r, pprhip_graph* g, int32_t src_internal, double eps, const pprhip_fora_conf_t* conf,
               uint64_t seed, int32_t* ids_out, double* vals_out, int cap) {
  return topk_begin_at(r, g, src_internal, nullptr, eps, conf, seed, ids_out, vals_out, cap);
}

// the same query from a seed set: the push session starts from p (the live seeds parked, as {s} is for one source)
int topk_begin_seeds(ForaRun& r, pprhip_graph* g, SeedTable& plan, double eps, const pprhip_fora_conf_t* conf,
                     uint64_t seed, int32_t* ids_out, double* vals_out, int cap) {
  return topk_begin_at(r, g, -1, &plan, eps, conf, seed, ids_out, vals_out, cap);
}

// the counters of a push that ran ahead, once its round is taken
void add_push_stats(pprhip_stats_t& sum, const pprhip_stats_t& st) {
  sum.pops += st.pops; sum.edge_pushes += st.edge_pushes; sum.enqueues += st.enqueues;
  sum.dense_nodes += st.dense_nodes; sum.dense_edges += st.dense_edges;
  sum.levels += st.levels; sum.dense_levels += st.dense_levels;
  sum.sweep_min_bytes += st.sweep_min_bytes; sum.push_bytes += st.push_bytes;
}

// The second stream of pprhip_fora_topk (make_side_stream picks one that runs beside the compute stream), its host
// mail, its plan record buffer and its events.
static int ensure_spec(pprhip_graph* g) {
  if (g->spec_stream) return PPRHIP_OK;
  if (g->spec_failed) return PPRHIP_ERR_STATE;
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (prio_lo == prio_hi) return PPRHIP_ERR_STATE;  // no second queue to be had: the rounds run one after another
  if (!g->spec_mail) {
    if (hipHostMalloc((void**)&g->spec_mail, sizeof(HostMail), hipHostMallocMapped) != hipSuccess) {
      (void)hipGetLastError();
      g->spec_mail = nullptr;
      return PPRHIP_ERR_OOM;
    }
    std::memset(g->spec_mail, 0, sizeof(HostMail));
  }
  if (hipHostGetDevicePointer((void**)&g->spec_mail_dev, g->spec_mail, 0) != hipSuccess) return PPRHIP_ERR_HIP;
  if (!g->mc_plan_rec2 && alloc_dev((void**)&g->mc_plan_rec2, sizeof(WalkPlanRec) * (size_t)g->gr->n) != PPRHIP_OK) {
    g->mc_plan_rec2 = nullptr;
    return PPRHIP_ERR_OOM;
  }
  for (auto& e : g->spec_ev)
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      e = nullptr;
      return PPRHIP_ERR_HIP;
    }
  PPRHIP_TRY(make_side_stream(g, &g->spec_stream));
  if (!g->spec_stream) {
    g->spec_failed = true;  // no stream of this process runs beside the compute stream: the rounds run in order
    return PPRHIP_ERR_STATE;
  }
  return PPRHIP_OK;
}

// While it lives, the handle launches on its second stream, reads back through that stream's mail and the calling
// thread times with that stream's timer.
struct SpecContext {
  pprhip_graph* g;
  hipStream_t stream;
  HostMail *mail, *mail_dev;
  unsigned long long seq;
  KernelTimer* timer;
  explicit SpecContext(pprhip_graph* g_) : g(g_), stream(g_->stream), mail(g_->mail), mail_dev(g_->mail_dev), seq(g_->mail_seq), timer(g_timer_cur) {
    g->stream = g->spec_stream;
    g->mail = g->spec_mail;
    g->mail_dev = g->spec_mail_dev;
    g->mail_seq = g->spec_mail_seq;
    g->spec_timer.stream = g->spec_stream;
    g->spec_timer.off = true;  // (its kernels run beside the compute stream's: their time is not the query's)
    g_timer_cur = &g->spec_timer;
  }
  ~SpecContext() {
    g->spec_mail_seq = g->mail_seq;
    g->stream = stream;
    g->mail = mail;
    g->mail_dev = mail_dev;
    g->mail_seq = seq;
    g_timer_cur = timer;
  }
};

// The next round's push, residue sum and walk plan (at delta_next), queued on the second stream behind the point where
// this round's walks have read the residues and the reserve (spec_ev[0]); spec_ev[1] marks its end.
int push_ahead(ForaRun& r, double delta_next, pprhip_stats_t& st_ahead) {
  pprhip_graph* g = r.g;
  SpecContext ctx(g);  // g->stream, the mail and the calling thread's timer are the second stream's until it ends
  PPRHIP_CHECK_HIP(hipStreamWaitEvent(g->stream, g->spec_ev[0], 0));
  r.ahead_pending = true;  // (from the first launch on the second stream on)
  PPRHIP_TRY(fetch_small(g, &g->ctr->dead_pops, &r.dead_before_ahead, sizeof r.dead_before_ahead));
  PushArgs a;
  LevelCtx L;
  bool pushing = false;  // (always: a query whose source is a dead end ends before its first round)
  PPRHIP_TRY(topk_push_start(g, r.sched.min_rmax, r.sched.push_rmax(r.sched.rmax(delta_next)), a, L, &pushing));
  PPRHIP_TRY(run_levels(g, a, L, st_ahead, nullptr));
  PPRHIP_TRY(launch_sum_partial(g, g->residue, act_n(g)));
  PPRHIP_TRY(launch_walk_plan(g, 1, r.alpha, 0.0, 0, g->est, r.sched.omega(delta_next)));
  PPRHIP_CHECK_HIP(hipEventRecord(g->spec_ev[1], g->stream));
  return PPRHIP_OK;
}

int topk_step(ForaRun& r, bool yield_dense) {
  pprhip_graph* g = r.g;
  const pprhip_fora_conf_t* conf = r.conf;
  const TopkSchedule& sc = r.sched;
  const size_t nd = sizeof(double) * (size_t)act_n(g);  // (est beyond the query's scan bound is zero and stays so)
  for (;;) {
    if (r.phase == ForaRun::kTopkRoundStart) {
      if (!(r.delta_local >= sc.min_delta)) {  // :123
        r.phase = ForaRun::kTopkFinal;
        continue;
      }
      r.rmax_local = sc.rmax(r.delta_local);    // :124
      r.omega_local = sc.omega(r.delta_local);  // :125
      // :126-132; a seed set whose seeds are all dead ends: the estimate is p (the reserve its start writes)
      if (r.seeded ? g->seeds->n_live == 0 : hdeg_out(g, r.src) == 0) {
        PPRHIP_CHECK_HIP(hipMemsetAsync(g->est, 0, nd, g->stream));
        if (!r.seeded) {
          PPRHIP_TRY(launch_set_f64(g, g->est, (uint32_t)r.src, 1.0));
        } else {
          PPRHIP_TRY(launch_seed_init(g, 0, true));
          PPRHIP_CHECK_HIP(hipMemcpyAsync(g->est, g->reserve, nd, hipMemcpyDeviceToDevice, g->stream));
        }
        r.rsum_local = 0.0;
        r.dead_src = true;
        r.phase = ForaRun::kTopkFinal;
        continue;
      }
      r.rmax_local = sc.push_rmax(r.rmax_local);  // :133
      if (r.marks) (void)hipEventRecord(g->ev[1], g->stream);
      if (r.pushed_ahead) {
        PPRHIP_CHECK_HIP(hipStreamWaitEvent(g->stream, g->spec_ev[1], 0));
        r.ahead_pending = false;
        r.phase = ForaRun::kTopkRoundEnd;
      } else {
        // forward_push_topk (:137; Forward_Push.java:144-250)
        bool pushing = false;  // (always: the dead-source case has ended the loop above)
        r.in_push = true;
        PPRHIP_TRY(topk_push_start(g, sc.min_rmax, r.rmax_local, r.a, r.L, &pushing));
        r.phase = ForaRun::kTopkLevels;
      }
    }
    if (r.phase == ForaRun::kTopkLevels) {
      const int rc = run_levels(g, r.a, r.L, r.st, nullptr, yield_dense);
      if (rc != PPRHIP_OK) return rc;  // kYield or an error
      leave_push(r);
      // :142-151 without a host round trip: the residue sum stays on the device, where the walk plan derives rsum and
      // the walk budget from it (:148,151); the sum reaches the host with the selection's read-back.  :143 the
      // estimate := copy of the push reserve (walk increments of earlier rounds are dropped), taken in the plan's pass
      PPRHIP_TRY(launch_sum_partial(g, g->residue, act_n(g)));  // (the plan adds the partial sums up)
      PPRHIP_TRY(launch_walk_plan(g, 1, r.alpha, 0.0, 0, g->est, r.omega_local, g->reserve, g->est));
      r.phase = ForaRun::kTopkRoundEnd;
    }
    if (r.phase == ForaRun::kTopkRoundEnd) {
      if (r.marks) (void)hipEventRecord(g->ev[2], g->stream);
      // a plan that ran ahead could not touch the estimate (the round before was still reading it): :143 here
      if (r.pushed_ahead) PPRHIP_CHECK_HIP(hipMemcpyAsync(g->est, g->reserve, nd, hipMemcpyDeviceToDevice, g->stream));
      r.pushed_ahead = false;
      if (r.ahead) PPRHIP_CHECK_HIP(hipEventRecord(g->spec_ev[0], g->stream));  // residues and reserve have been read
      // :155-168: the walk kernel reads the plan's counts on the device: no host round trip between push and selection
      const uint32_t waves = g->walk_waves;
      if (r.walk_waves) g->walk_waves = r.walk_waves;
      const int wrc = launch_walk_run(g, 1, r.alpha, r.seed, r.round, g->est);
      g->walk_waves = waves;
      PPRHIP_TRY(wrc);
      if (r.marks) (void)hipEventRecord(g->ev[3], g->stream);
      r.round++;
      unsigned long long sel_seq = 0;
      PPRHIP_TRY(select_launch(g, g->est, conf->k, &sel_seq, true));  // :173; the round's residue sum comes back with it
      // The next round's push, residue sum and walk plan run ahead of the decision whether there is a next round - but
      // not when this round is expected to be the last: at min_delta the loop ends whatever the selection says
      // (:175-176), and the k-th estimate hardly moves from round to round, so a round whose threshold the last k-th
      // value already meets is (almost always) final - its push ahead would be the largest of the query, and unused.
      const double delta_next = sc.next(r.delta_local);  // :178
      const bool likely_final = r.kth_prev >= 0.0 ? sc.last(r.kth_prev, r.delta_local) : r.delta_local <= sc.min_delta;
      pprhip_stats_t st_ahead;
      std::memset(&st_ahead, 0, sizeof st_ahead);
      const bool ahead = r.ahead && !likely_final;
      if (ahead) PPRHIP_TRY(push_ahead(r, delta_next, st_ahead));
      double kth = 0.0;
      bool have = false;
      PPRHIP_TRY(select_finish(g, sel_seq, g->est, conf->k, r.ids_out, r.vals_out, r.cap, &r.nsel, &kth, &have, r.st));
      g->topk_rsum = g->sel_plan_sum;  // (the sum this round's plan was derived from, in the selection's header)
      r.rsum_local = g->topk_rsum;     // :142
      if (!have) kth = 0.0;            // :174
      if (r.marks) {
        (void)hipEventRecord(g->ev[4], g->stream);
        PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
        r.push_ms += CallTimer::ms(g->ev[1], g->ev[2]);
        r.mc_ms += CallTimer::ms(g->ev[2], g->ev[3]);
        r.sel_ms += CallTimer::ms(g->ev[3], g->ev[4]);
      }
      r.st.kth_value = kth;
      r.kth_prev = kth;
      if (sc.last(kth, r.delta_local)) {  // :175-176
        r.ahead_discarded = ahead;
        r.phase = ForaRun::kTopkFinal;
        continue;
      }
      if (ahead) {  // the push ahead was this round's: its counters join the query's
        add_push_stats(r.st, st_ahead);
        r.pushed_ahead = true;
      }
      r.delta_local = delta_next;
      r.phase = ForaRun::kTopkRoundStart;
      continue;
    }
    if (r.phase == ForaRun::kTopkFinal) {
      if (r.round == 0 && !r.dead_src) PPRHIP_CHECK_HIP(hipMemsetAsync(g->est, 0, nd, g->stream));  // nothing ran
      g->result_in_est = true;
      if (r.ahead_discarded) {  // before the next query clears
        PPRHIP_CHECK_HIP(hipStreamWaitEvent(g->stream, g->spec_ev[1], 0));
        r.ahead_pending = false;
      }
      PPRHIP_TRY(read_dead_pops(g, r.st));
      if (r.ahead_discarded && r.st.dead_end_pops >= r.dead_before_ahead) {  // the unused push's dead-end pops are not the query's
        r.st.push_bytes -= 16ull * (r.st.dead_end_pops - r.dead_before_ahead);
        r.st.dead_end_pops = r.dead_before_ahead;
      }
      if (r.marks) (void)hipEventRecord(g->ev[3], g->stream);
      if (r.round == 0) {  // no round selected anything (the last round's selection is the result otherwise)
        bool have = false;
        double kth = 0.0;
        PPRHIP_TRY(select_topk(g, g->est, conf->k, r.ids_out, r.vals_out, r.cap, &r.nsel, &kth, &have, r.st));
      }
      if (r.marks) (void)hipEventRecord(g->ev[4], g->stream);
      r.st.rounds = r.round;
      r.st.rsum = r.rsum_local;
      r.st.rmax_final = r.rmax_local;
      r.st.omega = r.omega_local;
      r.phase = ForaRun::kDone;
    }
    return PPRHIP_OK;
  }
}

void add_stats(pprhip_stats_t& sum, const pprhip_stats_t& st) {
  sum.pops += st.pops; sum.edge_pushes += st.edge_pushes; sum.enqueues += st.enqueues;
  sum.dead_end_pops += st.dead_end_pops; sum.dense_nodes += st.dense_nodes; sum.dense_edges += st.dense_edges;
  sum.levels += st.levels;
  sum.dense_levels += st.dense_levels; sum.rounds += st.rounds; sum.mc_sources += st.mc_sources;
  sum.sweep_min_bytes += st.sweep_min_bytes;
  sum.walks += st.walks; sum.walk_steps += st.walk_steps; sum.select_passes += st.select_passes;
  sum.walk_loads += st.walk_loads; sum.walk_load_lanes += st.walk_load_lanes;
  sum.push_ms += st.push_ms; sum.mc_ms += st.mc_ms; sum.select_ms += st.select_ms; sum.total_ms += st.total_ms;
  sum.push_bytes += st.push_bytes; sum.mc_bytes += st.mc_bytes; sum.select_bytes += st.select_bytes;
  for (int c = 0; c < 8; ++c) {
    sum.class_ms[c] += st.class_ms[c];
    sum.class_bytes[c] += st.class_bytes[c];
    sum.class_launches[c] += st.class_launches[c];
  }
}

int run_step(ForaRun& r, bool yield_dense) {
  switch (r.kind) {
    case QueryKind::kBackward:
    case QueryKind::kPairs:
    case QueryKind::kTargets: return bwd_step(r, yield_dense);
    case QueryKind::kTopk: return topk_step(r, yield_dense);
    case QueryKind::kFora: break;
  }
  return fora_step(r, yield_dense);
}

}  // namespace detail
}  // namespace pprhip

int pprhip_fora_single_source(pprhip_graph_t* g, int32_t src, double eps, const pprhip_fora_conf_t* conf,
                              uint64_t seed, int n_rounds, double* reserve_out, pprhip_stats_t* stats) {
  PPRHIP_TRY(check_positive(eps, "pprhip_fora_single_source", "eps"));
  PPRHIP_TRY(check_conf(conf, "pprhip_fora_single_source", false));
  PPRHIP_TRY(check_graph(g, "pprhip_fora_single_source"));
  PPRHIP_TRY(check_node(g, src, "pprhip_fora_single_source"));
  src = g->gr->h_old2new[src];  // internal (degree-sorted) id
  if (!conf || !(eps > 0.0) || n_rounds < 0) {
    set_error("pprhip_fora_single_source: bad arguments (eps=%g n_rounds=%d)", eps, n_rounds);
    return PPRHIP_ERR_INVALID;
  }
  ForaRun r;
  PPRHIP_TRY(fora_begin(r, g, src, eps, conf, seed, n_rounds));
  CallTimer tm(g);
  r.tm = &tm;
  PPRHIP_TRY(fora_step(r, false));
  tm.finish(r.st);
  r.st.push_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  r.st.mc_ms = CallTimer::ms(g->ev[1], g->ev[2]);
  PPRHIP_TRY(copy_out(g, g->reserve, reserve_out));
  if (stats) *stats = r.st;
  return PPRHIP_OK;
}

// Fora_Whole_Graph.computeWholeGraphPPR from a seed set: the same rounds, thresholds, cost model and walks, the push
// started from p and its dead-end mass landed on p (seeds.cpp)
int pprhip_fora_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds, double eps,
                      const pprhip_fora_conf_t* conf, uint64_t seed, int n_rounds, double* reserve_out,
                      pprhip_stats_t* stats) {
  static const char* fn = "pprhip_fora_seeds";
  PPRHIP_TRY(check_positive(eps, fn, "eps"));
  PPRHIP_TRY(check_conf(conf, fn, false));
  PPRHIP_TRY(check_graph(g, fn));
  if (!conf || !(eps > 0.0) || n_rounds < 0) {
    set_error("%s: bad arguments (eps=%g n_rounds=%d)", fn, eps, n_rounds);
    return PPRHIP_ERR_INVALID;
  }
  SeedTable plan;
  PPRHIP_TRY(seed_plan(g, seeds, weights, n_seeds, conf->alpha, fn, plan));
  ForaRun r;
  PPRHIP_TRY(fora_begin_seeds(r, g, plan, eps, conf, seed, n_rounds));
  CallTimer tm(g);
  r.tm = &tm;
  {
    SeedScope scope(g);
    PPRHIP_TRY(fora_step(r, false));
  }
  tm.finish(r.st);
  r.st.push_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  r.st.mc_ms = CallTimer::ms(g->ev[1], g->ev[2]);
  PPRHIP_TRY(copy_out(g, g->reserve, reserve_out));
  if (stats) *stats = r.st;
  return PPRHIP_OK;
}

// ------------------------------------------------------------------ FORA top-k (a6)
// Fora_Topk.computeTopKPPR for one query, without yielding, on the run topk_begin* has just started.  A round's walks
// and selection do not touch what the next round's push works on (residue, reserve, frontier lists, parked flags: the
// plan has read the residues and the estimate is a copy of the reserve by then), and the next threshold is known
// beforehand (:178).  So while this round's walk kernel - bound by its longest walk, with most of the chip idle
//  - and selection run on the compute stream, the next round's push runs on a second stream, with
// counters of its own that only join the query's when the round turns out to be needed.  The one push that was not
// (after the last round) costs no time: it ends before that round's walks do.  PPRHIP_TOPK_AHEAD=0: the rounds run
// one after another, their phases timed by events.
static int fora_topk_drive(ForaRun& r, int* n_out, double* reserve_out, pprhip_stats_t* stats) {
  pprhip_graph* g = r.g;
  CallTimer tm(g);
  const char* spec_env = hook_env("PPRHIP_TOPK_AHEAD");
  r.ahead = !(spec_env && spec_env[0] == '0') && ensure_spec(g) == PPRHIP_OK;
  r.marks = !r.ahead;
  static const uint32_t topk_waves = [] {  // PPRHIP_TOPK_WALK_WAVES: measurement switch
    const char* e = hook_env("PPRHIP_TOPK_WALK_WAVES");
    return e && atoi(e) > 0 ? (uint32_t)atoi(e) : 8u;
  }();
  r.walk_waves = r.ahead ? topk_waves : 0u;  // (the next round's push runs beside these walks: leave it room)
  // A push queued ahead on the second stream works on this handle's residues, reserve and lists: whatever way this
  // function is left - an error return from any call below included - nothing may follow on the compute stream (the
  // next query's reset first of all) before that push has ended.  Joined: the compute stream waits for spec_ev[1]
  // (the round is taken, or the unused push is waited for at the end); otherwise the guard drains the second stream.
  struct SpecJoin {
    ForaRun& r;
    ~SpecJoin() {
      if (r.ahead_pending && r.g->spec_stream) (void)hipStreamSynchronize(r.g->spec_stream);
    }
  } spec_join{r};
  {
    SeedScope scope(g, r.seeded);
    PPRHIP_TRY(topk_step(r, false));
  }
  tm.finish(r.st);
  if (r.ahead) {  // phases of different rounds run side by side: the per-class kernel times stand for the phases
    r.st.push_ms = r.st.class_ms[PPRHIP_KERNEL_SPARSE_PUSH] + r.st.class_ms[PPRHIP_KERNEL_DENSE_PULL];
    r.st.mc_ms = r.st.class_ms[PPRHIP_KERNEL_WALK];
    r.st.select_ms = r.st.class_ms[PPRHIP_KERNEL_QUERY_SETUP];
  } else {
    r.st.push_ms = r.push_ms;
    r.st.mc_ms = r.mc_ms;
    r.st.select_ms = r.sel_ms + CallTimer::ms(g->ev[3], g->ev[4]);
  }
  if (n_out) *n_out = r.nsel;
  PPRHIP_TRY(copy_out(g, g->est, reserve_out));
  if (stats) *stats = r.st;
  return PPRHIP_OK;
}

int pprhip_fora_topk(pprhip_graph_t* g, int32_t src, double eps, const pprhip_fora_conf_t* conf, uint64_t seed,
                     int32_t* ids_out, double* vals_out, int cap, int* n_out, double* reserve_out,
                     pprhip_stats_t* stats) {
  PPRHIP_TRY(check_positive(eps, "pprhip_fora_topk", "eps"));
  PPRHIP_TRY(check_conf(conf, "pprhip_fora_topk", true));
  PPRHIP_TRY(check_graph(g, "pprhip_fora_topk"));
  PPRHIP_TRY(check_node(g, src, "pprhip_fora_topk"));
  if (!topk_args_ok(conf, eps, cap, ids_out, vals_out, "pprhip_fora_topk")) return PPRHIP_ERR_INVALID;
  ForaRun r;
  PPRHIP_TRY(topk_begin(r, g, g->gr->h_old2new[src], eps, conf, seed, ids_out, vals_out, cap));
  return fora_topk_drive(r, n_out, reserve_out, stats);
}

// pprhip_fora_topk from a seed set (seeds.cpp): the push session starts from p
int pprhip_fora_topk_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds, double eps,
                           const pprhip_fora_conf_t* conf, uint64_t seed, int32_t* ids_out, double* vals_out, int cap,
                           int* n_out, double* reserve_out, pprhip_stats_t* stats) {
  static const char* fn = "pprhip_fora_topk_seeds";
  PPRHIP_TRY(check_positive(eps, fn, "eps"));
  PPRHIP_TRY(check_conf(conf, fn, true));
  PPRHIP_TRY(check_graph(g, fn));
  if (!topk_args_ok(conf, eps, cap, ids_out, vals_out, fn)) return PPRHIP_ERR_INVALID;
  SeedTable plan;
  PPRHIP_TRY(seed_plan(g, seeds, weights, n_seeds, conf->alpha, fn, plan));
  ForaRun r;
  PPRHIP_TRY(topk_begin_seeds(r, g, plan, eps, conf, seed, ids_out, vals_out, cap));
  const int rc = fora_topk_drive(r, n_out, reserve_out, stats);
  g->topk_active = false;  // (no public round continues a seed-set session)
  return rc;
}
