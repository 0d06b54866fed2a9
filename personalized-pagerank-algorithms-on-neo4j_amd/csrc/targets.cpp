// targets.cpp — single-target PPR (beyond the reference): "who reaches t", for many targets and weighted target sets per
// call (include/pprhip.h "single targets", DESIGN.md §2 "Single targets").  The front of a target call, which
// pprhip_weighted_ppr_targets (weighted_bwd.cpp) shares - argument checks, the call's set table (duplicates merged,
// internal ids, in HBM) - and the entry point.  The pushes run as BatchJob kind kTargets of the batch driver
// (bwd_runs.cpp: target_begin / bwd_step), their start and the division by the survival vector S (pairs.cpp:
// ensure_survival) are kernels_target.hip; top-k, the result store and values_out are the driver's own delivery.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "engine_internal.hpp"

namespace pprhip {
namespace detail {

constexpr uint32_t kGroup = 8;  // a set starts on a multiple of this many table entries (kernels_target.hip: kTargetItems)

int target_plan(pprhip_graph_t* g, const int32_t* targets, const double* weights, const uint64_t* offsets, int q,
                double alpha, double rmax, pprhip_results* keep, int k, const int32_t* ids_out, const double* vals_out,
                pprhip_stats_t* stats_sum, const char* fn, bool weighted, TargetPlan& tp) {
  PPRHIP_TRY(check_alpha(alpha, fn));
  if (!(rmax > 0.0 && rmax <= 1.0)) {  // (NaN fails both)
    set_error("%s: rmax = %g must be finite with 0 < rmax <= 1", fn, rmax);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_graph(g, fn));
  if (weighted) PPRHIP_TRY(need_weights(g, fn));
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

  // the set table on the host: every set checked before anything runs
  tp.alpha = alpha;
  tp.rmax = rmax;
  std::vector<int32_t> h_id;
  std::vector<double> h_w;
  try {
    // a set is parsed as a seed set is - but the weights are NOT normalized - and then put in internal ids, ascending
    WeightedSet set;
    tp.first.reserve((size_t)q);
    for (int i = 0; i < q; ++i) {
      const uint64_t lo = offsets ? offsets[i] : (uint64_t)i, hi = offsets ? offsets[i + 1] : (uint64_t)i + 1;
      PPRHIP_TRY(parse_weighted_set(g->gr->n, targets + lo, weights ? weights + lo : nullptr, (int)(hi - lo), false,
                                    "target", fn, i, set));
      for (auto& x : set) x.first = g->gr->h_old2new[x.first];
      std::sort(set.begin(), set.end());  // (distinct ids: the weights never decide)
      uint32_t nf = 0;
      uint64_t ef = 0;
      for (const auto& x : set) {
        const uint32_t din = hdeg_in(g, x.first);
        if (din > 0 && x.second > rmax) {
          nf++;
          ef += din;
        }
      }
      tp.first.push_back(h_id.size());
      tp.count.push_back((uint32_t)set.size());
      tp.nf.push_back(nf);
      tp.ef.push_back(ef);
      tp.single.push_back(set.size() == 1 && set[0].second == 1.0 ? set[0].first : -1);
      tp.max_id.push_back(set.back().first);
      for (const auto& x : set) {
        h_id.push_back(x.first);
        h_w.push_back(x.second);
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

  // one device block for the call: the ids, then the weights on a 256-byte boundary
  const size_t b_id = sizeof(int32_t) * h_id.size(), b_w = sizeof(double) * h_w.size();
  const size_t off_w = (b_id + 255) & ~(size_t)255;
  PPRHIP_TRY(alloc_dev((void**)&tp.blob, off_w + b_w + 256));
  tp.d_id = reinterpret_cast<const int32_t*>(tp.blob);
  tp.d_w = reinterpret_cast<const double*>(tp.blob + off_w);
  if (hipMemcpyAsync(tp.blob, h_id.data(), b_id, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipMemcpyAsync(tp.blob + off_w, h_w.data(), b_w, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error("%s: upload of the target sets failed", fn);
    return PPRHIP_ERR_HIP;
  }
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip

using namespace pprhip;
using namespace pprhip::detail;

extern "C" int pprhip_ppr_targets(pprhip_graph_t* g, const int32_t* targets, const double* weights,
                                  const uint64_t* offsets, int q, double alpha, double rmax, pprhip_results_t* keep,
                                  double* values_out, int k, int32_t* ids_out, double* vals_out, int* n_out,
                                  pprhip_stats_t* per_query, pprhip_stats_t* stats_sum) {
  static const char* fn = "pprhip_ppr_targets";
  TargetPlan tp;
  PPRHIP_TRY(target_plan(g, targets, weights, offsets, q, alpha, rmax, keep, k, ids_out, vals_out, stats_sum, fn, false, tp));
  if (q == 0) return PPRHIP_OK;
  PPRHIP_TRY(ensure_survival(g, alpha));
  tp.survival = g->gr->survival;
  PPRHIP_TRY(ensure_batch(g));
  pprhip_stats_t sum;
  std::memset(&sum, 0, sizeof sum);
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
  J.alpha = alpha;
  J.threshold = rmax;
  J.targets = &tp;
  J.keep = keep;
  if (keep) keep->count = 0;
  PPRHIP_TRY(batch_run(g, J, &sum));
  if (keep) keep->count = q;
  if (stats_sum) {
    sum.rmax_final = rmax;
    *stats_sum = sum;
  }
  return PPRHIP_OK;
}
