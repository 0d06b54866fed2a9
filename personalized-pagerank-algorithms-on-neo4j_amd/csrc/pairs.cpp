// pairs.cpp — single-pair PPR (beyond the reference): the bidirectional estimator of include/pprhip.h "single pairs"
// (DESIGN.md §2 "Single pairs").  The front and back of a pair call, which pprhip_weighted_ppr_pairs (weighted_bwd.cpp)
// shares - argument checks, the grouping of a call's pairs by target, the call's device block, the read-back - the
// survival vector S that turns the backward push's leaking PPR into the engine's restarting one (kept on the lifted
// graph per alpha; its Jacobi driver serves the weighted S_w too), and the entry points.  The pushes and walks run as
// BatchJob kind kPairs of the batch driver (bwd_runs.cpp: pair_begin / bwd_step).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <numeric>
#include <vector>

#include "engine_internal.hpp"

namespace pprhip {
namespace detail {
namespace {

constexpr uint64_t kMaxPairWalks = 1ull << 48;   // walk indices carry 48 bits (kernels_walk.hip: counter word 2)
constexpr uint64_t kChunkWalks = 1024;           // walks per work item of k_pair_walk (16 per lane) ...
constexpr uint32_t kMaxChunks = 512;             // ... and at most this many items per pair (longer items beyond)
constexpr size_t kPartCap = (size_t)1 << 19;     // chunk sums per workspace (4 MB): pairs per walk launch = this / chunks
constexpr int kSurvivalCheck = 8;                // Jacobi iterations per convergence check
constexpr int kSurvivalMaxIters = 1 << 22;

int check_rmax_in(double rmax, const char* fn) {
  if (!(rmax >= 0.0 && rmax <= 1.0)) {  // (NaN fails both)
    set_error("%s: rmax = %g must be 0 (the default) or finite with 0 < rmax <= 1", fn, rmax);
    return PPRHIP_ERR_INVALID;
  }
  return PPRHIP_OK;
}

int pair_params(const pprhip_fora_conf_t* conf, double eps, double rmax_in, double* rmax_out, uint64_t* walks_out,
                double* omega_out, const char* fn) {
  const double lg = std::log(2.0 / conf->pfail);
  const double omega = 3.0 * lg / (eps * eps) / conf->delta;
  double rmax = rmax_in;
  if (!(rmax > 0.0)) {
    const double dbar = conf->n ? (double)conf->m / (double)conf->n : 0.0;
    rmax = eps * std::sqrt(dbar * conf->delta / (3.0 * lg));
    if (!(rmax > 0.0) || !std::isfinite(rmax)) rmax = 1.0;  // (no edges, or pfail >= 2: no balance to strike)
    rmax = std::min(rmax, 1.0);
  }
  const double w = omega > 0.0 ? std::ceil(omega * rmax) : 0.0;
  if (!(w < (double)kMaxPairWalks)) {
    set_error("%s: %g walks per pair (omega = %g, rmax = %g) exceed 2^48", fn, w, omega, rmax);
    return PPRHIP_ERR_INVALID;
  }
  if (rmax_out) *rmax_out = rmax;
  if (walks_out) *walks_out = (uint64_t)w;
  if (omega_out) *omega_out = omega;
  return PPRHIP_OK;
}

}  // namespace

int survival_jacobi(pprhip_graph* g, double alpha, const char* fn, bool both, bool converged,
                    const std::function<int(const double*, double*, unsigned long long*)>& iter, double** out) {
  const uint32_t n = g->gr->n;
  const size_t nd = sizeof(double) * (size_t)std::max<uint32_t>(n, 1);
  double* buf[2] = {nullptr, nullptr};
  unsigned long long* dmax = nullptr;
  int rc = alloc_dev((void**)&buf[0], nd);
  if (rc == PPRHIP_OK) rc = alloc_dev((void**)&buf[1], nd);
  if (rc == PPRHIP_OK) rc = alloc_dev((void**)&dmax, sizeof(unsigned long long));
  int cur = 0;
  if (rc == PPRHIP_OK && n) {
    std::vector<double> init(n, alpha);
    if (hipMemcpy(buf[0], init.data(), sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess ||
        (both && hipMemcpy(buf[1], init.data(), sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess)) {
      set_error("%s: upload of S0 failed", fn);
      rc = PPRHIP_ERR_HIP;
    }
  }
  bool done = converged;
  for (int it = 0; rc == PPRHIP_OK && !done && it < kSurvivalMaxIters; ++it) {
    const bool check = (it + 1) % kSurvivalCheck == 0;
    if (check && hipMemsetAsync(dmax, 0, sizeof(unsigned long long), g->stream) != hipSuccess) {
      set_error("%s: hipMemsetAsync failed", fn);
      rc = PPRHIP_ERR_HIP;
      break;
    }
    rc = iter(buf[cur], buf[cur ^ 1], check ? dmax : nullptr);
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
  if (rc != PPRHIP_OK && buf[cur]) (void)hipFree(buf[cur]);
  if (rc == PPRHIP_OK) *out = buf[cur];
  return rc;
}

// S at alpha on the lifted graph.  Runs on the calling thread, before any batch worker (GraphData is read-only while
// they run).
int ensure_survival(pprhip_graph* g, double alpha) {
  static const char* fn = "pprhip_walk_survival";
  GraphData* D = g->gr;
  if (D->survival && D->survival_alpha == alpha) return PPRHIP_OK;
  if (D->survival) (void)hipFree(D->survival);
  D->survival = nullptr;
  int32_t* d_heavy = nullptr;
  std::vector<int32_t> heavy;  // rows summed by a workgroup each (internal ids)
  for (uint32_t u = 0; u < D->n; ++u)
    if (D->h_out_rp[u + 1] - D->h_out_rp[u] >= survival_heavy_degree()) heavy.push_back((int32_t)u);
  if (!heavy.empty()) PPRHIP_TRY(alloc_dev((void**)&d_heavy, sizeof(int32_t) * heavy.size()));
  int rc = PPRHIP_OK;
  if (d_heavy && hipMemcpy(d_heavy, heavy.data(), sizeof(int32_t) * heavy.size(), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("%s: upload of S0 failed", fn);
    rc = PPRHIP_ERR_HIP;
  }
  if (rc == PPRHIP_OK)
    rc = survival_jacobi(g, alpha, fn, false, D->n == 0,
                         [&](const double* s_old, double* s_new, unsigned long long* dmax) {
                           return launch_survival_iter(g, s_old, s_new, alpha, d_heavy, (uint32_t)heavy.size(), dmax);
                         },
                         &D->survival);
  if (d_heavy) (void)hipFree(d_heavy);
  if (rc == PPRHIP_OK) D->survival_alpha = alpha;
  return rc;
}

int pair_plan(pprhip_graph_t* g, const int32_t* sources, const int32_t* targets, int q, double eps,
              const pprhip_fora_conf_t* conf, double rmax, uint64_t seed, const double* values_out,
              pprhip_stats_t* stats_sum, const char* fn, bool weighted, PairPlan& pp) {
  if (!conf) {
    set_error("%s: null conf", fn);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_conf(conf, fn, false));
  PPRHIP_TRY(check_positive(eps, fn, "eps"));
  PPRHIP_TRY(check_rmax_in(rmax, fn));
  PPRHIP_TRY(check_graph(g, fn));
  if (weighted) PPRHIP_TRY(need_weights(g, fn));
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
  PPRHIP_TRY(pair_params(conf, eps, rmax, &pp.rmax, &pp.walks, &pp.omega, fn));
  if (stats_sum) {
    std::memset(stats_sum, 0, sizeof *stats_sum);
    stats_sum->rmax_final = pp.rmax;
    stats_sum->omega = pp.omega;
  }
  if (q == 0) return PPRHIP_OK;
  pp.t0 = host_ms();
  pp.alpha = conf->alpha;
  pp.seed = seed;
  // pairs sorted by target (stable: the call order inside a target), one push per distinct target
  pp.order.resize((size_t)q);
  std::iota(pp.order.begin(), pp.order.end(), 0);
  std::stable_sort(pp.order.begin(), pp.order.end(), [&](int32_t a, int32_t b) { return targets[a] < targets[b]; });
  pp.h_src.resize((size_t)q);
  size_t max_group = 0;
  for (int j = 0; j < q; ++j) {
    const int32_t t = targets[pp.order[(size_t)j]];
    if (j == 0 || t != pp.distinct.back()) {
      if (j) max_group = std::max<size_t>(max_group, (size_t)j - pp.first.back());
      pp.distinct.push_back(t);
      pp.first.push_back((uint32_t)j);
    }
    pp.h_src[(size_t)j] = g->gr->h_old2new[sources[pp.order[(size_t)j]]];
  }
  max_group = std::max<size_t>(max_group, (size_t)q - pp.first.back());
  pp.first.push_back((uint32_t)q);
  pp.chunks = pp.walks ? (uint32_t)std::min<uint64_t>(kMaxChunks, (pp.walks + kChunkWalks - 1) / kChunkWalks) : 0u;
  pp.chunk_walks = pp.chunks ? (pp.walks + pp.chunks - 1) / pp.chunks : 0;
  pp.block_pairs = (uint32_t)std::max<size_t>(1, std::min(max_group, pp.chunks ? kPartCap / pp.chunks : max_group));
  pp.part_cap = std::max<size_t>(1, (size_t)pp.block_pairs * pp.chunks);
  return PPRHIP_OK;
}

int pair_upload(pprhip_graph* g, PairPlan& pp, int workspaces, int n_events, const char* fn) {
  // one device block for the call: sources, positions, values, steps counter, chunk sums of every workspace
  const size_t q = pp.order.size(), b_src = sizeof(int32_t) * q, b_val = sizeof(double) * q;
  const size_t off_pos = (b_src + 255) & ~(size_t)255, off_val = (off_pos + b_src + 255) & ~(size_t)255;
  const size_t off_steps = (off_val + b_val + 255) & ~(size_t)255, off_part = off_steps + 256;
  PPRHIP_TRY(alloc_dev((void**)&pp.blob, off_part + sizeof(double) * pp.part_cap * (size_t)workspaces));
  for (; pp.n_ev < n_events; ++pp.n_ev)
    if (hipEventCreate(&pp.ev[pp.n_ev]) != hipSuccess) {
      set_error("%s: hipEventCreate failed", fn);
      return PPRHIP_ERR_HIP;
    }
  pp.d_src = reinterpret_cast<const int32_t*>(pp.blob);
  pp.d_pos = reinterpret_cast<const int32_t*>(pp.blob + off_pos);
  pp.d_values = reinterpret_cast<double*>(pp.blob + off_val);
  pp.d_steps = reinterpret_cast<unsigned long long*>(pp.blob + off_steps);
  pp.d_part = reinterpret_cast<double*>(pp.blob + off_part);
  if (hipMemcpyAsync(pp.blob, pp.h_src.data(), b_src, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipMemcpyAsync(pp.blob + off_pos, pp.order.data(), b_src, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipMemsetAsync(pp.blob + off_steps, 0, 8, g->stream) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error("%s: upload of the pairs failed", fn);
    return PPRHIP_ERR_HIP;
  }
  return PPRHIP_OK;
}

int pair_collect(pprhip_graph* g, const PairPlan& pp, double* values_out, pprhip_stats_t& sum, pprhip_stats_t* stats_sum,
                 const char* fn) {
  unsigned long long steps = 0;
  if (hipMemcpyAsync(values_out, pp.d_values, sizeof(double) * pp.order.size(), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
      hipMemcpyAsync(&steps, pp.d_steps, sizeof steps, hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
      hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error("%s: read-back of the values failed", fn);
    return PPRHIP_ERR_HIP;
  }
  if (stats_sum) {
    sum.walk_steps = steps;
    sum.rmax_final = pp.rmax;
    sum.omega = pp.omega;
    sum.rounds = (uint32_t)pp.distinct.size();
    sum.total_ms = host_ms() - pp.t0;
    *stats_sum = sum;
  }
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip

using namespace pprhip;
using namespace pprhip::detail;

extern "C" {

int pprhip_pair_params(const pprhip_fora_conf_t* conf, double eps, double rmax_in, double* rmax_out, uint64_t* walks_out) {
  static const char* fn = "pprhip_pair_params";
  if (!conf) {
    set_error("%s: null conf", fn);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_conf(conf, fn, false));
  PPRHIP_TRY(check_positive(eps, fn, "eps"));
  PPRHIP_TRY(check_rmax_in(rmax_in, fn));
  return pair_params(conf, eps, rmax_in, rmax_out, walks_out, nullptr, fn);
}

int pprhip_walk_survival(pprhip_graph_t* g, double alpha, double* survival_out) {
  static const char* fn = "pprhip_walk_survival";
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(ensure_survival(g, alpha));
  return copy_out(g, g->gr->survival, survival_out);
}

int pprhip_ppr_pairs(pprhip_graph_t* g, const int32_t* sources, const int32_t* targets, int q, double eps,
                     const pprhip_fora_conf_t* conf, double rmax, uint64_t seed, double* values_out,
                     pprhip_stats_t* stats_sum) {
  static const char* fn = "pprhip_ppr_pairs";
  PairPlan pp;
  PPRHIP_TRY(pair_plan(g, sources, targets, q, eps, conf, rmax, seed, values_out, stats_sum, fn, false, pp));
  if (q == 0) return PPRHIP_OK;
  PPRHIP_TRY(ensure_survival(g, pp.alpha));
  pp.survival = g->gr->survival;
  PPRHIP_TRY(ensure_batch(g));
  PPRHIP_TRY(pair_upload(g, pp, kBatch, 3 * kBatch, fn));
  pprhip_stats_t sum;
  std::memset(&sum, 0, sizeof sum);
  BatchJob J;
  J.P = g;
  J.kind = QueryKind::kPairs;
  J.srcs = pp.distinct.data();
  J.q = (int)pp.distinct.size();
  J.eps = eps;
  J.conf = conf;
  J.seed = seed;
  J.alpha = pp.alpha;
  J.threshold = pp.rmax;
  J.pairs = &pp;
  PPRHIP_TRY(batch_run(g, J, &sum));
  return pair_collect(g, pp, values_out, sum, stats_sum, fn);
}

}  // extern "C"
