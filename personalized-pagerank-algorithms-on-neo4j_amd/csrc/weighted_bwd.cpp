// weighted_bwd.cpp — the backward direction over weighted relationships (include/pprhip.h "weighted relationships",
// DESIGN.md §2 "Weighted backward direction"): the weighted backward push, the weighted survival vector S_w, single
// targets / target sets and single pairs over P(u, v) = w / W(u), as a small driver of its own over
// kernels_weighted_bwd.hip - the mirror image of weighted.cpp.  The level loop is plain frontier-synchronous Jacobi,
// one level per host round trip, sparse or dense by the handle's dense_frac.  Weighted queries run one after another
// on the handle's own workspace: the 16-column batched sweeps are not shared.  Everything around a query is the
// unweighted engine's: the workspace and its reset, the start of a target set and the division by S
// (kernels_target.hip), the pair reduction (kernels_walk.hip), the delivery helpers, the getters.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

#include "run.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace {

constexpr uint32_t kGroup = 8;                  // a set starts on a multiple of this many table entries (kernels_target.hip)
constexpr uint64_t kChunkWalks = 1024;          // walks per work item of the pair walk kernel, as pairs.cpp ...
constexpr uint32_t kMaxChunks = 512;            // ... at most this many items per pair ...
constexpr size_t kPartCap = (size_t)1 << 19;    // ... and chunk sums per walk launch
constexpr int kSurvivalCheck = 8;               // Jacobi iterations per convergence check
constexpr int kSurvivalMaxIters = 1 << 22;

// ------------------------------------------------------------------ the level loop
struct WBLevels {
  int fcur = 0, ccur = 0, pslot = 0;
  uint32_t nf = 0;
  uint64_t ef = 0;
  bool prepared = false;  // the frontier is held as contributions in cdense[ccur] (after a dense level)
};

// Runs backward levels from the list L.fcur until the frontier is empty (weighted.cpp: run_weighted_levels, mirrored:
// no dead-end mass).  A level is dense when nodes + in-edges of its frontier reach dense_frac * m.
int run_weighted_bwd_levels(pprhip_graph* g, const PushArgs& a, WBLevels& L, pprhip_stats_t& st) {
  const unsigned long long dense_thresh = (unsigned long long)std::ceil(g->tun.dense_frac * (double)g->gr->m);
  const size_t nd = sizeof(double) * g->gr->n;
  unsigned long long* const list_counter = &g->ctr->hist[1];
  bool first_of_phase = false;
  while (L.nf > 0) {
    if ((unsigned long long)L.nf + L.ef >= dense_thresh) {
      if (!L.prepared) {  // list form -> contributions in place
        PPRHIP_TRY(ensure_bwd_layout(g));
        PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[L.ccur], 0, nd, g->stream));
        PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[L.ccur ^ 1], 0, nd, g->stream));
        PPRHIP_TRY(launch_wb_prepare(g, a, L.fcur, L.nf, true, L.ccur, nullptr));
        L.prepared = true;
        first_of_phase = true;
      }
      const uint64_t bytes = 12ull * g->gr->m + 8ull * g->gr->m + 40ull * g->gr->n_nz_o;
      ktimer().begin(PPRHIP_KERNEL_DENSE_PULL, bytes);
      PPRHIP_TRY(launch_wb_dense_level(g, a, L.ccur, L.pslot ^ 1));
      ktimer().end();
      // the sweep writes the contributions of the rows it applies only; a row without out-edges can hold one solely
      // from the phase's seeding, so the seeded buffer is cleared right after its first level has consumed it
      if (first_of_phase) PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[L.ccur], 0, nd, g->stream));
      first_of_phase = false;
      st.dense_levels++;
      st.levels++;
      st.dense_nodes += L.nf;
      st.dense_edges += L.ef;
      st.push_bytes += bytes;
      L.ccur ^= 1;
      L.pslot ^= 1;
      PPRHIP_TRY(fetch_packed(g, &g->ctr->packed[L.pslot], &L.nf, &L.ef));
      st.enqueues += L.nf;
      continue;
    }
    // ---- a sparse level
    uint32_t nf_list = L.nf;
    uint64_t ef_list = L.ef;
    ktimer().begin(PPRHIP_KERNEL_SPARSE_PUSH, 36ull * L.nf + 44ull * L.ef);
    if (L.prepared) {  // contributions in place -> list
      PPRHIP_CHECK_HIP(hipMemsetAsync(&g->ctr->hist[0], 0, 2 * sizeof(unsigned long long), g->stream));
      PPRHIP_TRY(launch_compact_prepared(g, L.ccur, L.fcur, &g->ctr->hist[0], true));
      PPRHIP_TRY(fetch_packed(g, &g->ctr->hist[0], &nf_list, &ef_list));
      L.prepared = false;
    } else {
      PPRHIP_TRY(launch_wb_prepare(g, a, L.fcur, L.nf, false, 0, list_counter));
    }
    PPRHIP_TRY(launch_wb_push(g, a, L.fcur, nf_list, ef_list, list_counter));
    ktimer().end();
    st.pops += L.nf;
    st.edge_pushes += L.ef;
    st.levels++;
    st.push_bytes += 36ull * L.nf + 44ull * L.ef;
    L.fcur ^= 1;
    PPRHIP_TRY(fetch_packed(g, list_counter, &L.nf, &L.ef));
    st.enqueues += L.nf;
  }
  return PPRHIP_OK;
}

// The push from one target (internal id) on a workspace just reset: r(t) = 1 and t pops unconditionally first.  A
// target without in-edges gets reserve(t) = lone_value and no push (*lone): 1.0 for pprhip_weighted_backward_push,
// alpha for targets and pairs (bwd_runs.cpp: backward_start).
int weighted_bwd_single(pprhip_graph* g, int32_t t, double alpha, double rmax, double lone_value, pprhip_stats_t& st,
                        bool* lone) {
  *lone = hdeg_in(g, t) == 0;
  if (*lone) return launch_set_f64(g, g->reserve, (uint32_t)t, lone_value);
  const PushArgs a{alpha, rmax, 0.0, t, kBackward};
  WBLevels L;
  PPRHIP_TRY(launch_set_f64(g, g->residue, (uint32_t)t, 1.0));
  PPRHIP_TRY(launch_seed_one(g, L.fcur, t));
  L.nf = 1;
  L.ef = hdeg_in(g, t);
  return run_weighted_bwd_levels(g, a, L, st);
}

// S_w at alpha on the lifted graph: Jacobi from S0 = alpha, double-buffered, on the handle's stream, until
// (1 - alpha) / alpha * max|dS| <= 1e-14 (pairs.cpp: ensure_survival).  Kept per alpha beside the unweighted S; goes
// with the weights (free_weights).
int ensure_weighted_survival(pprhip_graph* g, double alpha) {
  static const char* fn = "pprhip_weighted_walk_survival";
  GraphData* D = g->gr;
  if (D->wsurvival && D->wsurvival_alpha == alpha) return PPRHIP_OK;
  PPRHIP_TRY(ensure_bwd_layout(g));
  const size_t nd = sizeof(double) * (size_t)std::max<uint32_t>(D->n, 1);
  if (D->wsurvival) (void)hipFree(D->wsurvival);
  D->wsurvival = nullptr;
  double* buf[2] = {nullptr, nullptr};
  unsigned long long* dmax = nullptr;
  int rc = alloc_dev((void**)&buf[0], nd);
  if (rc == PPRHIP_OK) rc = alloc_dev((void**)&buf[1], nd);
  if (rc == PPRHIP_OK) rc = alloc_dev((void**)&dmax, sizeof(unsigned long long));
  int cur = 0;
  if (rc == PPRHIP_OK) {  // both buffers: the rows without out-edges keep alpha in either
    std::vector<double> init(D->n, alpha);
    if (hipMemcpy(buf[0], init.data(), sizeof(double) * D->n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(buf[1], init.data(), sizeof(double) * D->n, hipMemcpyHostToDevice) != hipSuccess) {
      set_error("%s: upload of S0 failed", fn);
      rc = PPRHIP_ERR_HIP;
    }
  }
  bool done = D->m == 0;
  for (int it = 0; rc == PPRHIP_OK && !done && it < kSurvivalMaxIters; ++it) {
    const bool check = (it + 1) % kSurvivalCheck == 0;
    if (check && hipMemsetAsync(dmax, 0, sizeof(unsigned long long), g->stream) != hipSuccess) {
      set_error("%s: hipMemsetAsync failed", fn);
      rc = PPRHIP_ERR_HIP;
      break;
    }
    rc = launch_wb_survival_iter(g, buf[cur], buf[cur ^ 1], alpha, check ? dmax : nullptr);
    cur ^= 1;
    if (rc != PPRHIP_OK || !check) continue;
    unsigned long long bits = 0;
    if (hipMemcpyAsync(&bits, dmax, sizeof bits, hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
        hipStreamSynchronize(g->stream) != hipSuccess) {
      set_error("%s: read-back of max|dS| failed", fn);
      rc = PPRHIP_ERR_HIP;
      break;
    }
    double dx;
    std::memcpy(&dx, &bits, 8);
    done = (1.0 - alpha) / alpha * dx <= 1e-14;
  }
  if (rc == PPRHIP_OK && !done) {
    set_error("%s: no convergence after %d iterations at alpha = %g", fn, kSurvivalMaxIters, alpha);
    rc = PPRHIP_ERR_STATE;
  }
  if (rc == PPRHIP_OK && hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error("%s: stream sync failed", fn);
    rc = PPRHIP_ERR_HIP;
  }
  if (dmax) (void)hipFree(dmax);
  if (buf[cur ^ 1]) (void)hipFree(buf[cur ^ 1]);
  if (rc != PPRHIP_OK) {
    if (buf[cur]) (void)hipFree(buf[cur]);
    return rc;
  }
  D->wsurvival = buf[cur];
  D->wsurvival_alpha = alpha;
  return PPRHIP_OK;
}

double host_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

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
  PPRHIP_TRY(check_alpha(alpha, fn));
  if (!(rmax > 0.0 && rmax <= 1.0)) {  // (NaN fails both)
    set_error("%s: rmax = %g must be finite with 0 < rmax <= 1", fn, rmax);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  if (q < 0 || k < 0 || (q > 0 && !targets) || (k > 0 && q > 0 && (!ids_out || !vals_out))) {
    set_error("%s: bad arguments (q=%d k=%d, targets %s)", fn, q, k, targets ? "given" : "NULL");
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_keep(keep, g, q, fn));
  if (q > 0 && offsets) PPRHIP_TRY(check_set_offsets(offsets, q, fn));
  if (stats_sum) {
    std::memset(stats_sum, 0, sizeof *stats_sum);
    stats_sum->rmax_final = rmax;
  }
  if (q == 0) {
    if (keep) keep->count = 0;
    return PPRHIP_OK;
  }

  // the set table on the host, as pprhip_ppr_targets builds it: every set checked before anything runs
  struct SetRec {
    uint64_t first;
    uint32_t count, nf;
    uint64_t ef;
    int32_t single, max_id;
  };
  std::vector<SetRec> sets;
  std::vector<int32_t> h_id;
  std::vector<double> h_w;
  try {
    WeightedSet set;
    sets.reserve((size_t)q);
    for (int i = 0; i < q; ++i) {
      const uint64_t lo = offsets ? offsets[i] : (uint64_t)i, hi = offsets ? offsets[i + 1] : (uint64_t)i + 1;
      PPRHIP_TRY(parse_weighted_set(g->gr->n, targets + lo, weights ? weights + lo : nullptr, (int)(hi - lo), false,
                                    "target", fn, i, set));
      for (auto& x : set) x.first = g->gr->h_old2new[x.first];
      std::sort(set.begin(), set.end());
      SetRec r{h_id.size(), (uint32_t)set.size(), 0u, 0ull,
               set.size() == 1 && set[0].second == 1.0 ? set[0].first : -1, set.back().first};
      for (const auto& x : set) {
        const uint32_t din = hdeg_in(g, x.first);
        if (din > 0 && x.second > rmax) {
          r.nf++;
          r.ef += din;
        }
        h_id.push_back(x.first);
        h_w.push_back(x.second);
      }
      while (h_id.size() % kGroup) {  // (never read as members: the kernel stops at the set's count)
        h_id.push_back(0);
        h_w.push_back(0.0);
      }
      sets.push_back(r);
    }
  } catch (const std::bad_alloc&) {
    set_error("%s: out of host memory for the table of %d target sets", fn, q);
    return PPRHIP_ERR_OOM;
  }

  PPRHIP_TRY(ensure_weighted_survival(g, alpha));
  const double* const surv = g->gr->wsurvival;
  // one device block for the call: the ids, then the weights on a 256-byte boundary
  const size_t b_id = sizeof(int32_t) * h_id.size(), b_w = sizeof(double) * h_w.size();
  const size_t off_w = (b_id + 255) & ~(size_t)255;
  char* blob = nullptr;
  PPRHIP_TRY(alloc_dev((void**)&blob, off_w + b_w + 256));
  const int32_t* const d_id = reinterpret_cast<const int32_t*>(blob);
  const double* const d_w = reinterpret_cast<const double*>(blob + off_w);
  int rc = PPRHIP_OK;
  if (hipMemcpyAsync(blob, h_id.data(), b_id, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipMemcpyAsync(blob + off_w, h_w.data(), b_w, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error("%s: upload of the target sets failed", fn);
    rc = PPRHIP_ERR_HIP;
  }
  pprhip_stats_t sum;
  std::memset(&sum, 0, sizeof sum);
  g->topk_active = false;
  if (keep) keep->count = 0;
  const size_t n = g->gr->n;
  // one set at a time on the handle's own workspace
  auto run_set = [&](int i) -> int {
    const SetRec& s = sets[(size_t)i];
    pprhip_stats_t st;
    std::memset(&st, 0, sizeof st);
    CallTimer tm(g);
    PPRHIP_TRY(reset_query_state(g, false, s.max_id));
    const double t0 = host_ms();
    bool lone = false;
    if (s.single >= 0) {
      PPRHIP_TRY(weighted_bwd_single(g, s.single, alpha, rmax, alpha, st, &lone));
    } else {
      const PushArgs a{alpha, rmax, 0.0, -1, kBackward};
      WBLevels L;
      // (the counter is zero: reset_query_state cleared the counters)
      PPRHIP_TRY(launch_target_init(g, d_id + s.first, d_w + s.first, s.count, L.fcur, &g->ctr->hist[kMaxBatch + 2], alpha,
                                    rmax));
      L.nf = s.nf;
      L.ef = s.ef;
      PPRHIP_TRY(run_weighted_bwd_levels(g, a, L, st));
    }
    st.push_ms = host_ms() - t0;
    PPRHIP_TRY(launch_target_finish(g, surv, act_n(g), lone ? s.single : -1));  // value = p / S_w in place of the reserve
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
    return PPRHIP_OK;
  };
  for (int i = 0; rc == PPRHIP_OK && i < q; ++i) rc = run_set(i);
  if (rc == PPRHIP_OK && hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error("%s: stream sync failed", fn);
    rc = PPRHIP_ERR_HIP;
  }
  (void)hipFree(blob);
  if (rc != PPRHIP_OK) return rc;
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
  if (!conf) {
    set_error("%s: null conf", fn);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_conf(conf, fn, false));
  PPRHIP_TRY(check_positive(eps, fn, "eps"));
  if (!(rmax >= 0.0 && rmax <= 1.0)) {  // (NaN fails both)
    set_error("%s: rmax = %g must be 0 (the default) or finite with 0 < rmax <= 1", fn, rmax);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  if (q < 0 || (q > 0 && (!sources || !targets || !values_out))) {
    set_error("%s: bad arguments (q=%d)", fn, q);
    return PPRHIP_ERR_INVALID;
  }
  for (int i = 0; i < q; ++i) {
    if (sources[i] < 0 || (uint32_t)sources[i] >= g->gr->n) {
      set_error("%s: pair %d: source id %d outside [0, %u)", fn, i, sources[i], g->gr->n);
      return PPRHIP_ERR_INVALID;
    }
    if (targets[i] < 0 || (uint32_t)targets[i] >= g->gr->n) {
      set_error("%s: pair %d: target id %d outside [0, %u)", fn, i, targets[i], g->gr->n);
      return PPRHIP_ERR_INVALID;
    }
  }
  // r_max and w are pprhip_pair_params', unchanged (dbar = m / n, the relationship count)
  double rmax_used = 0.0;
  uint64_t walks = 0;
  PPRHIP_TRY(pprhip_pair_params(conf, eps, rmax, &rmax_used, &walks));
  const double omega = 3.0 * std::log(2.0 / conf->pfail) / (eps * eps) / conf->delta;
  if (stats_sum) {
    std::memset(stats_sum, 0, sizeof *stats_sum);
    stats_sum->rmax_final = rmax_used;
    stats_sum->omega = omega;
  }
  if (q == 0) return PPRHIP_OK;
  const auto t0 = std::chrono::steady_clock::now();
  const double alpha = conf->alpha;
  // pairs sorted by target (stable: the call order inside a target), one push per distinct target
  std::vector<int32_t> order((size_t)q);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return targets[a] < targets[b]; });
  std::vector<int32_t> h_src((size_t)q), distinct;
  std::vector<uint32_t> first;
  size_t max_group = 0;
  for (int j = 0; j < q; ++j) {
    const int32_t t = targets[order[(size_t)j]];
    if (j == 0 || t != distinct.back()) {
      if (j) max_group = std::max<size_t>(max_group, (size_t)j - first.back());
      distinct.push_back(t);
      first.push_back((uint32_t)j);
    }
    h_src[(size_t)j] = g->gr->h_old2new[sources[order[(size_t)j]]];
  }
  max_group = std::max<size_t>(max_group, (size_t)q - first.back());
  first.push_back((uint32_t)q);
  const uint32_t chunks = walks ? (uint32_t)std::min<uint64_t>(kMaxChunks, (walks + kChunkWalks - 1) / kChunkWalks) : 0u;
  const uint64_t chunk_walks = chunks ? (walks + chunks - 1) / chunks : 0;
  const uint32_t block_pairs = (uint32_t)std::max<size_t>(1, std::min(max_group, chunks ? kPartCap / chunks : max_group));
  const size_t part_cap = std::max<size_t>(1, (size_t)block_pairs * chunks);

  PPRHIP_TRY(ensure_weighted_survival(g, alpha));
  const double* const surv = g->gr->wsurvival;
  // one device block for the call: sources, positions, values, steps counter, chunk sums
  const size_t b_src = sizeof(int32_t) * (size_t)q, b_val = sizeof(double) * (size_t)q;
  const size_t off_pos = (b_src + 255) & ~(size_t)255, off_val = (off_pos + b_src + 255) & ~(size_t)255;
  const size_t off_steps = (off_val + b_val + 255) & ~(size_t)255, off_part = off_steps + 256;
  char* blob = nullptr;
  PPRHIP_TRY(alloc_dev((void**)&blob, off_part + sizeof(double) * part_cap));
  const int32_t* const d_src = reinterpret_cast<const int32_t*>(blob);
  const int32_t* const d_pos = reinterpret_cast<const int32_t*>(blob + off_pos);
  double* const d_values = reinterpret_cast<double*>(blob + off_val);
  unsigned long long* const d_steps = reinterpret_cast<unsigned long long*>(blob + off_steps);
  double* const d_part = reinterpret_cast<double*>(blob + off_part);
  int rc = PPRHIP_OK;
  if (hipMemcpyAsync(blob, h_src.data(), b_src, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipMemcpyAsync(blob + off_pos, order.data(), b_src, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipMemsetAsync(blob + off_steps, 0, 8, g->stream) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error("%s: upload of the pairs failed", fn);
    rc = PPRHIP_ERR_HIP;
  }
  pprhip_stats_t sum;
  std::memset(&sum, 0, sizeof sum);
  g->topk_active = false;
  auto run_target = [&](size_t i) -> int {
    const int32_t t = g->gr->h_old2new[distinct[i]];
    const uint32_t lo = first[i], hi = first[i + 1];
    pprhip_stats_t st;
    std::memset(&st, 0, sizeof st);
    CallTimer tm(g);
    PPRHIP_TRY(reset_query_state(g, false, t));
    tm.mark(1);
    bool lone = false;
    PPRHIP_TRY(weighted_bwd_single(g, t, alpha, rmax_used, alpha, st, &lone));
    tm.mark(2);
    // a target without in-edges left no residue: its values are exact, no walks
    const uint32_t ch = lone ? 0u : chunks;
    ktimer().begin(PPRHIP_KERNEL_WALK, 0);
    for (uint32_t b = lo; b < hi; b += block_pairs) {
      const uint32_t np = std::min(block_pairs, hi - b);
      if (ch) PPRHIP_TRY(launch_wb_pair_walk(g, d_src + b, np, ch, chunk_walks, walks, alpha, seed, d_part, d_steps));
      PPRHIP_TRY(launch_pair_reduce(g, d_src + b, d_pos + b, np, ch, d_part, walks, surv, d_values));
    }
    ktimer().end();
    tm.mark(3);
    tm.finish(st);
    st.push_ms = CallTimer::ms(g->ev[1], g->ev[2]);
    st.mc_ms = CallTimer::ms(g->ev[2], g->ev[3]);
    if (ch) {
      st.walks += walks * (uint64_t)(hi - lo);
      st.mc_sources += hi - lo;
    }
    add_stats(sum, st);
    return PPRHIP_OK;
  };
  for (size_t i = 0; rc == PPRHIP_OK && i < distinct.size(); ++i) rc = run_target(i);
  unsigned long long steps = 0;
  if (rc == PPRHIP_OK &&
      (hipMemcpyAsync(values_out, d_values, b_val, hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
       hipMemcpyAsync(&steps, d_steps, sizeof steps, hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
       hipStreamSynchronize(g->stream) != hipSuccess)) {
    set_error("%s: read-back of the values failed", fn);
    rc = PPRHIP_ERR_HIP;
  }
  (void)hipFree(blob);
  if (rc != PPRHIP_OK) return rc;
  if (stats_sum) {
    sum.walk_steps = steps;
    sum.rmax_final = rmax_used;
    sum.omega = omega;
    sum.rounds = (uint32_t)distinct.size();
    sum.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *stats_sum = sum;
  }
  return PPRHIP_OK;
}

}  // extern "C"
