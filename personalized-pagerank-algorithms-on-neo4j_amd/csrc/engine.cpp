// engine.cpp — the single-query C ABI of the pprhip engine: kernel timing, tuning and conf functions, top-k push
// rounds, top-k select, Monte-Carlo, backward push and the power method, with the parameter checks every entry point
// runs and the top-k push session.  Everything numerical runs in the HIP kernels; the host only sequences launches on
// the handle's stream.  The forward push and walk-batch calls live in forward_calls.cpp, the handle's lifecycle in
// graph.cpp, the level loop in levels.cpp, the selection driver in select.cpp, read-backs and walk launchers in
// device_io.cpp, FORA runs in fora.cpp, the runs that push backward in bwd_runs.cpp, the batched entry points in
// batch.cpp, batch_api.cpp and stream.cpp, All-Pair in allpair.cpp and its index in index.cpp (shared declarations:
// engine_internal.hpp).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace pprhip {
namespace detail {

int copy_out(pprhip_graph* g, const double* dev, double* host) {
  if (!host) return PPRHIP_OK;
  const double* srcp = dev;
  if (g->gr->relabeled) {  // back to the caller's ids: out[old] = x[old2new[old]]
    PPRHIP_TRY(launch_permute_out(g, dev, g->cF));
    srcp = g->cF;
  }
  PPRHIP_CHECK_HIP(hipMemcpyAsync(host, srcp, sizeof(double) * g->gr->n, hipMemcpyDeviceToHost, g->stream));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  return PPRHIP_OK;
}

int check_graph(const pprhip_graph* g, const char* fn) {
  if (!g) {
    set_error("%s: null graph handle", fn);
    return PPRHIP_ERR_INVALID;
  }
  if (g->stream_open) {
    set_error("%s: a query stream is open on this handle (pprhip_fora_stream_close first)", fn);
    return PPRHIP_ERR_STATE;
  }
  hipError_t e = hipSetDevice(g->gr->device);
  if (e != hipSuccess) {
    set_error("%s: hipSetDevice(%d) failed: %s", fn, g->gr->device, hipGetErrorString(e));
    return PPRHIP_ERR_NO_DEVICE;
  }
  return PPRHIP_OK;
}

int check_node(const pprhip_graph* g, int32_t v, const char* fn) {
  if (!node_in_range(g, v)) {
    set_error("%s: node id %d outside [0, %u)", fn, v, g->gr->n);
    return PPRHIP_ERR_INVALID;
  }
  return PPRHIP_OK;
}

// Range checks of the numeric parameters (include/pprhip.h, "Parameter ranges").  Every entry point runs them before
// check_graph, so an out-of-range value is refused without a device and never reaches a kernel: at alpha <= 0 a walk
// never stops and a push on a cycle never ends, at alpha = 1 rmax0 divides by zero, at eps <= 0 the walk count omega
// is infinite.  NaN fails every test below.
int check_alpha(double alpha, const char* fn, const char* name) {
  if (!(alpha > 0.0 && alpha < 1.0)) {
    set_error("%s: %s = %g outside (0, 1)", fn, name, alpha);
    return PPRHIP_ERR_INVALID;
  }
  return PPRHIP_OK;
}

int check_positive(double v, const char* fn, const char* name) {
  if (!(v > 0.0 && std::isfinite(v))) {
    set_error("%s: %s = %g must be finite and > 0", fn, name, v);
    return PPRHIP_ERR_INVALID;
  }
  return PPRHIP_OK;
}

int check_threshold(double v, const char* fn, const char* name) {
  if (!(v >= 0.0 && std::isfinite(v))) {
    set_error("%s: %s = %g must be finite and >= 0", fn, name, v);
    return PPRHIP_ERR_INVALID;
  }
  return PPRHIP_OK;
}

int check_conf(const pprhip_fora_conf_t* c, const char* fn, bool topk) {
  if (!c) return PPRHIP_OK;  // (the entry point's own null check reports it)
  PPRHIP_TRY(check_alpha(c->alpha, fn, "conf->alpha"));
  PPRHIP_TRY(check_positive(c->delta, fn, "conf->delta"));
  if (!topk) return check_positive(c->pfail, fn, "conf->pfail");
  // pprhip_conf_fora_topk's own degenerate values pass: pfail = +inf at n div k = 1 and -0 at k > n
  if (std::isnan(c->pfail) || c->pfail < 0.0) {
    set_error("%s: conf->pfail = %g must be > 0", fn, c->pfail);
    return PPRHIP_ERR_INVALID;
  }
  return check_positive(c->min_delta, fn, "conf->min_delta");
}

bool topk_args_ok(const pprhip_fora_conf_t* conf, double eps, int cap, const int32_t* ids_out, const double* vals_out,
                  const char* fn) {
  if (!conf || conf->k < 1 || !(eps > 0.0) || cap < 0 || (cap > 0 && (!ids_out || !vals_out))) {
    set_error("%s: bad arguments", fn);
    return false;
  }
  return true;
}

int check_set_offsets(const uint64_t* offsets, int q, const char* fn) {
  if (offsets[0] != 0) {
    set_error("%s: offsets[0] = %llu, not 0", fn, (unsigned long long)offsets[0]);
    return PPRHIP_ERR_INVALID;
  }
  for (int i = 0; i < q; ++i)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > (uint64_t)INT32_MAX) {
      set_error("%s: set %d: offsets %llu .. %llu do not describe a set", fn, i, (unsigned long long)offsets[i],
                (unsigned long long)offsets[i + 1]);
      return PPRHIP_ERR_INVALID;
    }
  return PPRHIP_OK;
}

int check_keep(const pprhip_results* keep, const pprhip_graph* g, int q, const char* fn) {
  if (keep && (keep->g != g || q > keep->capacity)) {
    set_error("%s: the result store belongs to another graph or holds %d < %d queries", fn, keep->capacity, q);
    return PPRHIP_ERR_INVALID;
  }
  return PPRHIP_OK;
}

int parse_weighted_set(uint32_t n, const int32_t* ids_in, const double* weights, int k, bool normalize, const char* noun,
                       const char* fn, int set, WeightedSet& e) {
  e.clear();
  const auto where = [&] { return set < 0 ? std::string(fn) : std::string(fn) + ": set " + std::to_string(set); };
  const auto refused = [&] {  // (after set_error)
    e.clear();
    return PPRHIP_ERR_INVALID;
  };
  if (k <= 0 || !ids_in) {
    set_error("%s: a %s set needs at least one %s (n_%ss=%d)", where().c_str(), noun, noun, noun, k);
    return refused();
  }
  e.reserve((size_t)k);
  for (int i = 0; i < k; ++i) {
    const int32_t v = ids_in[i];
    if (v < 0 || (uint32_t)v >= n) {
      set_error("%s: %s %d: node id %d outside [0, %u)", where().c_str(), noun, i, v, n);
      return refused();
    }
    const double w = weights ? weights[i] : 1.0;
    if (!std::isfinite(w) || w < 0.0) {
      set_error("%s: %s %d: weight %g is not a finite non-negative number", where().c_str(), noun, i, w);
      return refused();
    }
    e.push_back({v, w});
  }
  std::sort(e.begin(), e.end(), [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& b) {
    return a.first < b.first;
  });
  double sum = 0.0;
  for (const auto& x : e) sum += x.second;
  if (!(sum > 0.0) || !std::isfinite(sum)) {
    set_error("%s: the %s weights sum to %g", where().c_str(), noun, sum);
    return refused();
  }
  size_t kept = 0;
  for (size_t i = 0; i < e.size();) {  // duplicates are summed, zero weights dropped (in place: kept <= i)
    size_t j = i;
    double w = 0.0;
    for (; j < e.size() && e[j].first == e[i].first; ++j) w += e[j].second;
    if (w > 0.0) e[kept++] = {e[i].first, normalize ? w / sum : w};
    i = j;
  }
  e.resize(kept);
  return PPRHIP_OK;
}

uint32_t hdeg_out(const pprhip_graph* g, int32_t v) { return g->gr->h_out_rp[v + 1] - g->gr->h_out_rp[v]; }
uint32_t hdeg_in(const pprhip_graph* g, int32_t v) { return g->gr->h_in_rp[v + 1] - g->gr->h_in_rp[v]; }

// ------------------------------------------------------------------ the top-k push session
int topk_session_reset(pprhip_graph* g, int32_t src, SeedTable* plan, double alpha, double rsum) {
  PPRHIP_TRY(reset_query_state(g, true, plan ? plan->max_id : src));
  if (plan) PPRHIP_TRY(seed_upload(g, *plan));
  else PPRHIP_CHECK_HIP(hipMemsetAsync(g->flags + src, 1, 1, g->stream));  // Q = {s} (Fora_Topk.java:117-118): parked
  g->topk_active = true;
  g->topk_first = true;
  g->topk_src = plan ? -1 : src;
  g->topk_seeded = plan != nullptr;
  g->topk_alpha = alpha;
  g->topk_rsum = rsum;
  g->topk_dead_pops = 0;
  return PPRHIP_OK;
}

int topk_push_start(pprhip_graph* g, double min_rmax, double rmax, PushArgs& a, LevelCtx& L, bool* pushing) {
  const int32_t src = g->topk_src;  // (-1: a seed set, g->seeds)
  *pushing = false;
  if (!g->topk_seeded && hdeg_out(g, src) == 0) {  // Forward_Push.java:149-153
    PPRHIP_TRY(launch_set_f64(g, g->reserve, (uint32_t)src, 1.0));
    g->topk_rsum = 0.0;
    return PPRHIP_OK;
  }
  if (g->topk_first) {
    if (g->topk_seeded) PPRHIP_TRY(launch_seed_init(g, 0, true));  // r = p resolved, the live seeds parked
    else PPRHIP_TRY(launch_set_f64(g, g->residue, (uint32_t)src, 1.0));  // :155-156
    g->topk_first = false;
  }
  a = PushArgs{g->topk_alpha, rmax, min_rmax, src, kFwdTopk};
  L = LevelCtx();
  PPRHIP_TRY(seed_scan(g, a, 1, L));
  *pushing = true;
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int pprhip_set_kernel_timing(int on) {
  const int was = kernel_timing_level();
  g_kernel_timing.store(on == 2 ? 2 : (on ? 1 : 0), std::memory_order_relaxed);
  return was;
}

int pprhip_device_count(int* count_out) {
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) c = 0;
  if (count_out) *count_out = c;
  return PPRHIP_OK;
}

void pprhip_tuning_default(pprhip_tuning_t* t) {
  if (!t) return;
  // calibrated on MI355X; tests/test_host.py checks the test twin uses the same numbers
  t->c_walk_ns = 0.35;
  t->c_edge_ns = 0.06;
  t->c_pop_ns = 0.10;
  t->c_level_ns = 12000.0;
  t->c_dense_edge_ns = 0.012;
  t->c_dense_node_ns = 0.02;
  t->dense_frac = 0.05;
  t->max_rounds = 24;
  t->max_halvings = 6;
  t->halving_ratio = 2.0;
  t->prior_levels = 16;
  t->gs_blocks = 2;
  t->gs_frac = 0.1;
}

void pprhip_tuning_batch(pprhip_tuning_t* t) {
  pprhip_tuning_default(t);
  if (!t) return;
  // fitted on R-MAT 22 with all slots busy: a sweep of 1.6 ms serves ~14.5 queries; a level that touches
  // fewer than 2 % of the edges is cheaper as a sparse level (one memory-side atomic per edge)
  t->c_dense_edge_ns = 0.002;
  t->c_dense_node_ns = 0.003;
  t->dense_frac = 0.02;
  t->gs_frac = 0.05;
}

// The single and the batch profile for a handle that carries a walk index (pprhip_walk_index_build): equal to the
// profiles they start from, because c_walk_ns at the measured cost of a served walk lost (DESIGN.md §2 "Walk index").
void pprhip_tuning_indexed(pprhip_tuning_t* t) { pprhip_tuning_default(t); }

void pprhip_tuning_indexed_batch(pprhip_tuning_t* t) { pprhip_tuning_batch(t); }

// The batch profile for a call of q queries on one GPU (config #4's shares: 50 queries over 8 GPUs are 6-7 per call).  A
// sweep costs the same whatever the number of busy columns, so a dense level costs each query of a small call more:
// the dense constants and the level-shape thresholds scale with 14.5 / min(q, 14.5) columns, up to the single-query
// profile's values (a call of one IS the single-query path).  Chosen by the caller before the first query starts, so
// every query of the call is pprhip_fora_single_source under the same tuning.
void pprhip_tuning_batch_for(int q, pprhip_tuning_t* t) {
  pprhip_tuning_batch(t);
  if (!t || q >= 15) return;
  pprhip_tuning_t one;
  pprhip_tuning_default(&one);
  const double scale = 14.5 / (double)std::max(1, q);
  t->c_dense_edge_ns = std::min(one.c_dense_edge_ns, t->c_dense_edge_ns * scale);
  t->c_dense_node_ns = std::min(one.c_dense_node_ns, t->c_dense_node_ns * scale);
  t->dense_frac = std::min(one.dense_frac, t->dense_frac * scale);
  t->gs_frac = std::min(one.gs_frac, t->gs_frac * scale);
}

int pprhip_conf_fora_whole_graph(uint32_t n, uint64_t m, double alpha, pprhip_fora_conf_t* c) {
  PPRHIP_TRY(check_alpha(alpha, "pprhip_conf_fora_whole_graph"));
  if (!c || n == 0) {
    set_error("pprhip_conf_fora_whole_graph: bad arguments");
    return PPRHIP_ERR_INVALID;
  }
  std::memset(c, 0, sizeof *c);
  c->alpha = alpha;
  c->delta = 1.0 / (double)n;  // Algo_Conf.java:47
  c->pfail = 1.0 / (double)n;  // :48
  c->rsum = 1.0;               // :49
  c->n = n;
  c->m = m;
  return PPRHIP_OK;
}

int pprhip_conf_fora_topk(uint32_t n, uint64_t m, int k, double alpha, pprhip_fora_conf_t* c) {
  PPRHIP_TRY(check_alpha(alpha, "pprhip_conf_fora_topk"));
  if (!c || n == 0 || k < 1) {
    set_error("pprhip_conf_fora_topk: bad arguments (n=%u k=%d)", n, k);
    return PPRHIP_ERR_INVALID;
  }
  std::memset(c, 0, sizeof *c);
  c->alpha = alpha;
  c->min_delta = 1.0 / (double)n;  // Algo_Conf.java:73
  c->k = k;
  c->delta = 1.0 / (double)k;  // :75
  c->pfail = 1.0 / (double)n / (double)n / std::log((double)((int32_t)n / k));  // :76 (int division)
  c->rsum = 1.0;
  c->n = n;
  c->m = m;
  return PPRHIP_OK;
}

int pprhip_fora_whole_params(const pprhip_fora_conf_t* c, double eps, double* rmax0, double* omega) {
  PPRHIP_TRY(check_positive(eps, "pprhip_fora_whole_params", "eps"));
  PPRHIP_TRY(check_conf(c, "pprhip_fora_whole_params", false));
  if (!c || !rmax0 || !omega) {
    set_error("pprhip_fora_whole_params: null argument");
    return PPRHIP_ERR_INVALID;
  }
  *rmax0 = eps * std::sqrt(c->delta / 3.0 / (double)c->m / std::log(2.0 / c->pfail)) / (1.0 - c->alpha);
  *omega = (eps + 2.0) * std::log(2.0 / c->pfail) / eps / eps / c->delta;
  return PPRHIP_OK;
}

int pprhip_fora_topk_params(const pprhip_fora_conf_t* c, double eps, double delta, double* min_rmax,
                            double* rmax_scaled, double* omega) {
  PPRHIP_TRY(check_positive(eps, "pprhip_fora_topk_params", "eps"));
  PPRHIP_TRY(check_positive(delta, "pprhip_fora_topk_params", "delta"));
  PPRHIP_TRY(check_conf(c, "pprhip_fora_topk_params", true));
  if (!c || !min_rmax || !rmax_scaled || !omega) {
    set_error("pprhip_fora_topk_params: null argument");
    return PPRHIP_ERR_INVALID;
  }
  const double e = eps * 0.5;  // Fora_Topk.java:109-110
  *min_rmax = e * std::sqrt(c->min_delta / 3 / (double)c->m / std::log(2 / c->pfail));  // :113
  double rmax = e * std::sqrt(delta / 3.0 / (double)c->m / std::log(2.0 / c->pfail));     // :124
  *omega = (e + 2.0) * std::log(2.0 / c->pfail) / e / e / delta;                           // :125
  rmax *= std::sqrt((double)c->m * rmax) * 3.0;                                            // :133
  *rmax_scaled = rmax;
  return PPRHIP_OK;
}

// ------------------------------------------------------------------ resumable top-k push (a2)
int pprhip_fwdpush_topk_reset(pprhip_graph_t* g, int32_t src, double alpha) {
  PPRHIP_TRY(check_alpha(alpha, "pprhip_fwdpush_topk_reset"));
  PPRHIP_TRY(check_graph(g, "pprhip_fwdpush_topk_reset"));
  PPRHIP_TRY(check_node(g, src, "pprhip_fwdpush_topk_reset"));
  return topk_session_reset(g, g->gr->h_old2new[src], nullptr, alpha, 1.0);
}

int pprhip_fwdpush_topk_round(pprhip_graph_t* g, double min_rmax, double rmax, double* rsum_out,
                              pprhip_stats_t* stats) {
  PPRHIP_TRY(check_threshold(min_rmax, "pprhip_fwdpush_topk_round", "min_rmax"));
  PPRHIP_TRY(check_threshold(rmax, "pprhip_fwdpush_topk_round", "rmax"));
  PPRHIP_TRY(check_graph(g, "pprhip_fwdpush_topk_round"));
  if (!g->topk_active) {
    set_error("pprhip_fwdpush_topk_round: call pprhip_fwdpush_topk_reset first");
    return PPRHIP_ERR_STATE;
  }
  pprhip_stats_t st;
  std::memset(&st, 0, sizeof st);
  CallTimer tm(g);
  {
    SeedScope scope(g, g->topk_seeded);
    PushArgs a;
    LevelCtx L;
    bool pushing = false;
    PPRHIP_TRY(topk_push_start(g, min_rmax, rmax, a, L, &pushing));
    if (pushing) {
      PPRHIP_TRY(run_levels(g, a, L, st, nullptr));
      PPRHIP_TRY(device_sum(g, g->residue, &g->topk_rsum));
    }
  }
  // the device counts dead-end pops since the reset; a round reports its own, as it reports every other counter
  st.dead_end_pops = g->topk_dead_pops;
  PPRHIP_TRY(read_dead_pops(g, st));
  const uint64_t dead_seen = st.dead_end_pops;
  st.dead_end_pops = dead_seen >= g->topk_dead_pops ? dead_seen - g->topk_dead_pops : dead_seen;
  g->topk_dead_pops = dead_seen;
  tm.mark(1);
  tm.finish(st);
  st.push_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  st.rsum = g->topk_rsum;
  st.rmax_final = rmax;
  st.rounds = 1;
  if (rsum_out) *rsum_out = g->topk_rsum;
  if (stats) *stats = st;
  return PPRHIP_OK;
}

// ------------------------------------------------------------------ top-k select (a7)
int pprhip_topk_select(pprhip_graph_t* g, int k, int32_t* ids_out, double* vals_out, int cap, int* n_out,
                       double* kth_out, pprhip_stats_t* stats) {
  PPRHIP_TRY(check_graph(g, "pprhip_topk_select"));
  if (k < 1 || cap < 0 || !n_out || (cap > 0 && (!ids_out || !vals_out))) {
    set_error("pprhip_topk_select: bad arguments (k=%d cap=%d)", k, cap);
    return PPRHIP_ERR_INVALID;
  }
  pprhip_stats_t st;
  std::memset(&st, 0, sizeof st);
  CallTimer tm(g);
  bool have = false;
  PPRHIP_TRY(select_topk(g, g->result_in_est ? g->est : g->reserve, k, ids_out, vals_out, cap, n_out, kth_out, &have,
                         st));
  tm.mark(1);
  tm.finish(st);
  st.select_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  if (stats) *stats = st;
  return PPRHIP_OK;
}

// ------------------------------------------------------------------ pure Monte-Carlo
int pprhip_monte_carlo(pprhip_graph_t* g, int32_t src, double eps, const pprhip_fora_conf_t* conf, uint64_t seed,
                       double* ppr_out, pprhip_stats_t* stats) {
  PPRHIP_TRY(check_positive(eps, "pprhip_monte_carlo", "eps"));
  PPRHIP_TRY(check_conf(conf, "pprhip_monte_carlo", false));
  PPRHIP_TRY(check_graph(g, "pprhip_monte_carlo"));
  PPRHIP_TRY(check_node(g, src, "pprhip_monte_carlo"));
  src = g->gr->h_old2new[src];  // internal (degree-sorted) id
  if (!conf) {
    set_error("pprhip_monte_carlo: bad arguments");
    return PPRHIP_ERR_INVALID;
  }
  pprhip_stats_t st;
  std::memset(&st, 0, sizeof st);
  g->topk_active = false;
  PPRHIP_TRY(reset_query_state(g, false, src));
  CallTimer tm(g);
  const double omega = 3 * std::log(2 / conf->pfail) / eps / eps / conf->delta;  // Monte_Carlo.java:145
  const uint64_t nw = (uint64_t)std::floor(omega);                                // :149 (i <= omega)
  if (nw >= (1ull << kPackShift)) {
    set_error("pprhip_monte_carlo: %llu walks exceed the engine's 2^36 limit", (unsigned long long)nw);
    return PPRHIP_ERR_INVALID;
  }
  if (hdeg_out(g, src) == 0) {
    PPRHIP_TRY(launch_set_f64(g, g->reserve, (uint32_t)src, (double)nw / omega));  // every walk returns src (:70-72)
    st.walks = nw;
  } else {
    ktimer().begin(PPRHIP_KERNEL_WALK, 0);
    PPRHIP_TRY(launch_mc_pure(g, src, nw, conf->alpha, seed, 1.0 / omega, g->reserve));
    ktimer().end();
    PPRHIP_TRY(read_dead_pops(g, st));  // steps, walks (= nw), sources (= 1) as the device counted them
  }
  st.mc_sources = 1;
  st.omega = omega;
  tm.mark(1);
  tm.finish(st);
  st.mc_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  PPRHIP_TRY(copy_out(g, g->reserve, ppr_out));
  if (stats) *stats = st;
  return PPRHIP_OK;
}

// ------------------------------------------------------------------ backward search (a8)
static int backward_push_impl(pprhip_graph_t* g, int32_t target, double alpha, double rmax, pprhip_stats_t& st) {
  PPRHIP_TRY(reset_query_state(g, false, target));
  PushArgs a;
  LevelCtx L;
  bool pushing = false;
  PPRHIP_TRY(backward_start(g, L, a, target, alpha, rmax, 1.0, &pushing));
  return pushing ? run_levels(g, a, L, st, nullptr) : PPRHIP_OK;
}

int pprhip_backward_push(pprhip_graph_t* g, int32_t target, double alpha, double rmax, double* reserve_out,
                         double* residue_out, pprhip_stats_t* stats) {
  PPRHIP_TRY(check_alpha(alpha, "pprhip_backward_push"));
  PPRHIP_TRY(check_threshold(rmax, "pprhip_backward_push", "rmax"));
  PPRHIP_TRY(check_graph(g, "pprhip_backward_push"));
  PPRHIP_TRY(check_node(g, target, "pprhip_backward_push"));
  target = g->gr->h_old2new[target];  // internal (degree-sorted) id
  pprhip_stats_t st;
  std::memset(&st, 0, sizeof st);
  g->topk_active = false;
  CallTimer tm(g);
  PPRHIP_TRY(backward_push_impl(g, target, alpha, rmax, st));
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

// ------------------------------------------------------------------ ground truth (a12)
int pprhip_power_method(pprhip_graph_t* g, int32_t src, double alpha, int iters, double* reserve_out,
                        pprhip_stats_t* stats) {
  PPRHIP_TRY(check_alpha(alpha, "pprhip_power_method"));
  if (iters < 0) {
    set_error("pprhip_power_method: iters = %d must be >= 0", iters);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_graph(g, "pprhip_power_method"));
  PPRHIP_TRY(check_node(g, src, "pprhip_power_method"));
  src = g->gr->h_old2new[src];  // internal (degree-sorted) id
  pprhip_stats_t st;
  std::memset(&st, 0, sizeof st);
  g->topk_active = false;
  PPRHIP_TRY(reset_query_state(g, false, src));
  CallTimer tm(g);
  if (iters > 0) {
    // iteration 1 (Power_Method.java:59-96 with residue = {s: 1})
    PPRHIP_TRY(ensure_panel_part(g));
    LevelCtx L;
    PushArgs a{alpha, 0.0, 0.0, src, kPower};
    PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[L.ccur], 0, sizeof(double) * g->gr->n, g->stream));
    PPRHIP_TRY(launch_set_f64(g, g->reserve, (uint32_t)src, 1.0 * alpha));
    const uint32_t d = hdeg_out(g, src);
    const double remain = 1.0 * (1 - alpha);
    if (d == 0)
      PPRHIP_TRY(launch_set_f64(g, &g->ctr->dead[L.dslot], 0, remain));
    else
      PPRHIP_TRY(launch_set_f64(g, g->cdense[L.ccur], (uint32_t)src, remain / (double)d));
    for (int it = 1; it < iters; ++it) {
      const int out = L.pslot ^ 1;
      PPRHIP_TRY(launch_dense_pull(g, a, L.ccur, out, L.dslot, it == 1));
      L.ccur ^= 1;
      L.dslot ^= 1;
      L.pslot = out;
      st.dense_levels++;
      st.levels++;
      st.push_bytes += dense_level_bytes(g);
      st.sweep_min_bytes += dense_level_min_bytes(g);
    }
  }
  tm.mark(1);
  tm.finish(st);
  st.push_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  st.rounds = (uint32_t)iters;
  PPRHIP_TRY(copy_out(g, g->reserve, reserve_out));
  if (stats) *stats = st;
  return PPRHIP_OK;
}

#ifdef PPRHIP_TEST_HOOKS
// Test / tuning hook (libpprhip_hooks.so only): the edge kernel of block `block` of `n_blocks` Gauss-Seidel blocks of a
// batched forward sweep (n_blocks <= 1: the whole sweep), `reps` launches back to back; average microseconds per launch.
int pprhip_hook_time_sweep_edges(pprhip_graph_t* g, int block, int n_blocks, int reps, double* us_out) {
  if (!g || !us_out || reps <= 0 || g->parent) {
    set_error("pprhip_hook_time_sweep_edges: bad arguments");
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_CHECK_HIP(hipSetDevice(g->gr->device));
  PPRHIP_TRY(ensure_batch(g));
  GsBlock B{0u, g->gr->n_nz, 0ull, (unsigned long long)g->gr->m};
  if (n_blocks > 1) {
    pprhip_tuning_t keep = g->batch->slots[0]->tun;
    g->batch->slots[0]->tun.gs_blocks = n_blocks;
    int nb = 1;
    const GsBlock* blocks = gs_blocks_of(g->batch->slots[0], &nb);
    g->batch->slots[0]->tun = keep;
    if (!blocks || block < 0 || block >= nb) {
      set_error("pprhip_hook_time_sweep_edges: no block %d of %d", block, n_blocks);
      return PPRHIP_ERR_INVALID;
    }
    B = blocks[block];
  }
  hipEvent_t e0, e1;
  PPRHIP_CHECK_HIP(hipEventCreate(&e0));
  PPRHIP_CHECK_HIP(hipEventCreate(&e1));
  PPRHIP_TRY(launch_sweep_edges_only(g, B));  // warm-up
  PPRHIP_CHECK_HIP(hipEventRecord(e0, g->stream));
  for (int i = 0; i < reps; ++i) PPRHIP_TRY(launch_sweep_edges_only(g, B));
  PPRHIP_CHECK_HIP(hipEventRecord(e1, g->stream));
  PPRHIP_CHECK_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  PPRHIP_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *us_out = (double)ms * 1e3 / reps;
  // (the row-major kernel adds into acc8 with atomics where rows cross chunks: start the next sweep clean)
  PPRHIP_CHECK_HIP(hipMemsetAsync(g->batch->acc8, 0, sizeof(double) * ((size_t)g->gr->n + 1) * kBatch, g->stream));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  return PPRHIP_OK;
}
#endif

}  // extern "C"

// (All-Pair's whole-vector searches, allpair.cpp)
int pprhip::detail::backward_search_whole(pprhip_graph_t* g, int32_t target, double alpha, double rmax, pprhip_stats_t& st) {
  return backward_push_impl(g, target, alpha, rmax, st);
}
