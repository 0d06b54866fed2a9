// targets.cpp — single-target PPR (beyond the reference): "who reaches t", for many targets and weighted target sets per
// call (include/pprhip.h "single targets", DESIGN.md §2 "Single targets").  Argument checks, the call's set table
// (duplicates merged, internal ids, in HBM) and the entry point.  The pushes run as BatchJob kind kTargets of the batch
// driver (fora.cpp: target_begin / target_step), their start and the division by the survival vector S (pairs.cpp:
// ensure_survival) are kernels_target.hip; top-k, the result store and values_out are the driver's own delivery.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace {

constexpr uint32_t kGroup = 8;  // a set starts on a multiple of this many table entries (kernels_target.hip: kTargetItems)

struct Member {
  int32_t v;
  double w;
};

// Set i of the call, checked by the seed-set rules (seed_normalize) - but the weights are NOT normalized - and merged
// into `out`: distinct internal ids ascending, duplicates summed, zero weights dropped.
int target_set(const pprhip_graph* g, const int32_t* ids, const double* weights, uint64_t count, int i, const char* fn,
               std::vector<Member>& out) {
  out.clear();
  const uint32_t n = g->gr->n;
  if (count == 0) {
    set_error("%s: set %d: a target set needs at least one target", fn, i);
    return PPRHIP_ERR_INVALID;
  }
  out.reserve((size_t)count);
  double sum = 0.0;
  for (uint64_t j = 0; j < count; ++j) {
    const int32_t v = ids[j];
    if (v < 0 || (uint32_t)v >= n) {
      set_error("%s: set %d: target %llu: node id %d outside [0, %u)", fn, i, (unsigned long long)j, v, n);
      return PPRHIP_ERR_INVALID;
    }
    const double w = weights ? weights[j] : 1.0;
    if (!std::isfinite(w) || w < 0.0) {
      set_error("%s: set %d: target %llu: weight %g is not a finite non-negative number", fn, i, (unsigned long long)j, w);
      return PPRHIP_ERR_INVALID;
    }
    sum += w;
    out.push_back({g->gr->h_old2new[v], w});
  }
  if (!(sum > 0.0) || !std::isfinite(sum)) {
    set_error("%s: set %d: the target weights sum to %g", fn, i, sum);
    return PPRHIP_ERR_INVALID;
  }
  std::sort(out.begin(), out.end(), [](const Member& a, const Member& b) { return a.v < b.v; });
  size_t k = 0;
  for (size_t a = 0; a < out.size();) {
    size_t b = a;
    double w = 0.0;
    for (; b < out.size() && out[b].v == out[a].v; ++b) w += out[b].w;
    if (w > 0.0) out[k++] = {out[a].v, w};
    a = b;
  }
  out.resize(k);
  return PPRHIP_OK;
}

}  // namespace

extern "C" int pprhip_ppr_targets(pprhip_graph_t* g, const int32_t* targets, const double* weights,
                                  const uint64_t* offsets, int q, double alpha, double rmax, pprhip_results_t* keep,
                                  double* values_out, int k, int32_t* ids_out, double* vals_out, int* n_out,
                                  pprhip_stats_t* per_query, pprhip_stats_t* stats_sum) {
  static const char* fn = "pprhip_ppr_targets";
  PPRHIP_TRY(check_alpha(alpha, fn));
  if (!(rmax > 0.0 && rmax <= 1.0)) {  // (NaN fails both)
    set_error("%s: rmax = %g must be finite with 0 < rmax <= 1", fn, rmax);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_graph(g, fn));
  if (q < 0 || k < 0 || (q > 0 && !targets) || (k > 0 && q > 0 && (!ids_out || !vals_out))) {
    set_error("%s: bad arguments (q=%d k=%d, targets %s)", fn, q, k, targets ? "given" : "NULL");
    return PPRHIP_ERR_INVALID;
  }
  if (keep && (keep->g != g || q > keep->capacity)) {
    set_error("%s: the result store belongs to another graph or holds %d < %d queries", fn, keep->capacity, q);
    return PPRHIP_ERR_INVALID;
  }
  if (q > 0 && offsets) {
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
  }
  if (stats_sum) {
    std::memset(stats_sum, 0, sizeof *stats_sum);
    stats_sum->rmax_final = rmax;
  }
  if (q == 0) {
    if (keep) keep->count = 0;
    return PPRHIP_OK;
  }

  // the set table on the host: every set checked before anything runs
  TargetPlan tp;
  tp.alpha = alpha;
  tp.rmax = rmax;
  std::vector<int32_t> h_id;
  std::vector<double> h_w;
  try {
    std::vector<Member> set;
    tp.first.reserve((size_t)q);
    for (int i = 0; i < q; ++i) {
      const uint64_t lo = offsets ? offsets[i] : (uint64_t)i, hi = offsets ? offsets[i + 1] : (uint64_t)i + 1;
      PPRHIP_TRY(target_set(g, targets + lo, weights ? weights + lo : nullptr, hi - lo, i, fn, set));
      uint32_t nf = 0;
      uint64_t ef = 0;
      for (const Member& x : set) {
        const uint32_t din = hdeg_in(g, x.v);
        if (din > 0 && x.w > rmax) {
          nf++;
          ef += din;
        }
      }
      tp.first.push_back(h_id.size());
      tp.count.push_back((uint32_t)set.size());
      tp.nf.push_back(nf);
      tp.ef.push_back(ef);
      tp.single.push_back(set.size() == 1 && set[0].w == 1.0 ? set[0].v : -1);
      tp.max_id.push_back(set.back().v);
      for (const Member& x : set) {
        h_id.push_back(x.v);
        h_w.push_back(x.w);
      }
      while (h_id.size() % kGroup) {  // (never read as members: the kernel stops at the set's count)
        h_id.push_back(0);
        h_w.push_back(0.0);
      }
    }
  } catch (const std::bad_alloc&) {
    set_error("%s: out of host memory for the table of %d target sets", fn, q);
    return PPRHIP_ERR_OOM;
  }

  PPRHIP_TRY(ensure_survival(g, alpha));
  tp.survival = g->gr->survival;
  PPRHIP_TRY(ensure_batch(g));
  // one device block for the call: the ids, then the weights on a 256-byte boundary
  const size_t b_id = sizeof(int32_t) * h_id.size(), b_w = sizeof(double) * h_w.size();
  const size_t off_w = (b_id + 255) & ~(size_t)255;
  char* blob = nullptr;
  PPRHIP_TRY(alloc_dev((void**)&blob, off_w + b_w + 256));
  tp.d_id = reinterpret_cast<const int32_t*>(blob);
  tp.d_w = reinterpret_cast<const double*>(blob + off_w);
  int rc = PPRHIP_OK;
  if (hipMemcpyAsync(blob, h_id.data(), b_id, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipMemcpyAsync(blob + off_w, h_w.data(), b_w, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error("%s: upload of the target sets failed", fn);
    rc = PPRHIP_ERR_HIP;
  }
  pprhip_stats_t sum;
  std::memset(&sum, 0, sizeof sum);
  if (rc == PPRHIP_OK) {
    BatchJob J;
    J.P = g;
    J.kind = QueryKind::kTargets;
    J.srcs = nullptr;
    J.q = q;
    J.eps = 0.0;
    J.conf = nullptr;
    J.seed = 0;
    J.n_rounds = 0;
    J.reserve_out = values_out;
    J.k = k;
    J.ids_out = ids_out;
    J.vals_out = vals_out;
    J.n_out = n_out;
    J.per_query = per_query;
    J.alpha = alpha;
    J.threshold = rmax;
    J.targets = &tp;
    J.keep = keep;
    if (keep) keep->count = 0;
    rc = batch_run(g, J, &sum);
    if (rc == PPRHIP_OK && keep) keep->count = q;
  }
  (void)hipFree(blob);
  if (rc != PPRHIP_OK) return rc;
  if (stats_sum) {
    sum.rmax_final = rmax;
    *stats_sum = sum;
  }
  return PPRHIP_OK;
}
