// weighted_sweep.cpp — weighted local clustering: the driver of the sweep cut by relationship weight
// (pprhip_weight_quantum, pprhip_weighted_sweep_cut, pprhip_results_weighted_sweep_cut,
// pprhip_weighted_local_cluster_seeds; include/pprhip.h "weighted local clustering", DESIGN.md §2 "Weighted sweep cut").
// It shares the handle's sweep workspace with sweep.cpp and sequences the same steps on the handle's stream - support,
// order, rank table and volumes, the edge scan, the best prefix - over kernels_weighted_sweep.hip and the steps of
// kernels_sweep.hip that are generic.  What depends on the weights alone (the shift, qdeg, the total volume) is built
// once per weight set and kept beside the weights.
#include <cmath>
#include <cstring>
#include <limits>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace {

// the quantum rule's shift from the largest weight and the number of weights (m >= 1)
int quantum_shift(double wmax, uint64_t m) {
  int e = 0;
  (void)std::frexp(wmax, &e);  // wmax = f * 2^e, 0.5 <= f < 1
  int L = 0;
  while (L < 64 && (1ull << L) < m) ++L;
  return 61 - e - L;
}

// the parameters and buffers, before the handle is looked at
int check_wsweep_args(const char* fn, int normalize, double max_vol, const void* a, const void* b, const void* c,
                      uint64_t cap, const pprhip_wsweep_t* info) {
  if (normalize != 0 && normalize != 1) {
    set_error("%s: normalize = %d must be 0 or 1", fn, normalize);
    return PPRHIP_ERR_INVALID;
  }
  if (!info) {
    set_error("%s: null info", fn);
    return PPRHIP_ERR_INVALID;
  }
  if (cap == 0 && (a || b || c)) {
    set_error("%s: an output buffer with cap = 0", fn);
    return PPRHIP_ERR_INVALID;
  }
  return check_threshold(max_vol, fn, "max_vol");
}

// qdeg, the shift and the total volume of the handle's weights, built when they are not there; w: the sweep workspace
// (three cells of its best-prefix scratch carry the maximum, the total and the number of hub rows, its tile_node the
// list of hub rows)
int ensure_quanta(pprhip_graph* g, SweepWs* w) {
  GraphData* D = g->gr;
  if (D->qdeg) return PPRHIP_OK;
  // both are idle before the support step.  The hub list takes two words of tile_node per row of kQdegHubRow entries
  // or more, and the rows' lengths add up to 2m
  if (2 * (2 * (uint64_t)D->m / kQdegHubRow) > (uint64_t)w->tile_cap) {
    set_error("weighted sweep: %zu tile words cannot hold the hub rows of %llu relationships", w->tile_cap,
              (unsigned long long)D->m);
    return PPRHIP_ERR_STATE;
  }
  unsigned long long* cells = w->part_idx;
  unsigned long long h[3] = {0, 0, 0};
  PPRHIP_CHECK_HIP(hipMemsetAsync(cells, 0, sizeof h, g->stream));
  PPRHIP_TRY(launch_wsweep_wmax(g, &cells[0]));
  PPRHIP_TRY(fetch_small(g, cells, h, sizeof h));
  double wmax = 0.0;
  std::memcpy(&wmax, &h[0], sizeof wmax);
  if (D->m && !(std::isfinite(wmax) && wmax > 0.0)) {
    set_error("weighted sweep: the largest relationship weight reads %g", wmax);
    return PPRHIP_ERR_STATE;
  }
  const int shift = D->m ? quantum_shift(wmax, D->m) : 0;
  unsigned long long* qdeg = nullptr;
  PPRHIP_TRY(alloc_dev((void**)&qdeg, sizeof(unsigned long long) * (size_t)D->n));
  int rc = launch_wsweep_qdeg(g, w, shift, qdeg, &cells[1], &cells[2]);
  if (!rc) rc = fetch_small(g, cells, h, sizeof h);
  if (!rc && h[1] > (1ull << 62)) {
    set_error("weighted sweep: a total volume of %llu quanta", h[1]);
    rc = PPRHIP_ERR_STATE;
  }
  if (rc) {
    (void)hipFree(qdeg);
    return rc;
  }
  D->qdeg = qdeg;
  D->q_shift = shift;
  D->q_total = h[1];
  D->qdeg_bytes = sizeof(unsigned long long) * (uint64_t)D->n;
  return PPRHIP_OK;
}

// max_vol in quanta: min(2^63 - 1, floor(max_vol * 2^s)); *bounded: max_vol > 0
uint64_t vol_limit(double max_vol, int shift, bool* bounded) {
  *bounded = max_vol > 0.0;
  if (!*bounded) return 0;
  const double t = std::floor(std::ldexp(max_vol, shift));
  return t >= 9223372036854775808.0 ? (uint64_t)std::numeric_limits<int64_t>::max() : (uint64_t)t;
}

// the sweep over x (internal order, n doubles in HBM); order / vol_q / cut_q stay in the workspace (wsweep_fetch)
int wsweep_run(pprhip_graph* g, const double* x, int normalize, uint64_t max_size, double max_vol, pprhip_wsweep_t* info) {
  std::memset(info, 0, sizeof *info);
  info->best_conductance = std::numeric_limits<double>::infinity();
  PPRHIP_TRY(ensure_sweep(g));
  SweepWs* w = g->sweep;
  if (!w->qvolx) PPRHIP_TRY(alloc_dev((void**)&w->qvolx, sizeof(unsigned long long) * ((size_t)g->gr->n + 1)));
  PPRHIP_TRY(ensure_quanta(g, w));
  const GraphData* D = g->gr;
  info->total_vol_q = D->q_total;
  info->shift = D->q_shift;
  bool bounded = false;
  const uint64_t limit = vol_limit(max_vol, D->q_shift, &bounded);
  PPRHIP_CHECK_HIP(hipEventRecord(g->ev[0], g->stream));
  PPRHIP_TRY(launch_wsweep_support(g, w, x, normalize));
  unsigned long long support = 0;
  PPRHIP_TRY(fetch_small(g, w->hdr, &support, sizeof support));
  if (support > D->n) {
    set_error("weighted sweep: %llu ranked nodes of %u", support, D->n);
    return PPRHIP_ERR_STATE;
  }
  info->support = support;
  const uint32_t profiled = (uint32_t)(max_size > 0 && max_size < support ? max_size : support);
  info->profiled = profiled;
  if (support) PPRHIP_TRY(launch_sweep_sort(g, w, (uint32_t)support));
  PPRHIP_CHECK_HIP(hipEventRecord(g->ev[1], g->stream));
  // a limit below one quantum admits no prefix (every ranked node has qdeg >= 1); 0 would read "no bound" below
  const bool any_admitted = !bounded || limit > 0;
  if (profiled) {
    PPRHIP_TRY(launch_wsweep_rank(g, w, profiled));
    PPRHIP_TRY(launch_wsweep_edges(g, w, profiled, g->ev[2], g->ev[3]));
    if (any_admitted) PPRHIP_TRY(launch_sweep_best_over(g, w, w->qvolx, w->cut, profiled, D->q_total, limit));
  }
  PPRHIP_CHECK_HIP(hipEventRecord(g->ev[5], g->stream));
  if (profiled) {
    unsigned long long hdr[kSweepHdrWords];
    PPRHIP_TRY(fetch_small(g, w->hdr, hdr, sizeof hdr));
    if (any_admitted) {
      info->best_size = hdr[1];
      info->best_cut_q = hdr[2];
      info->best_vol_q = hdr[3];
      std::memcpy(&info->best_conductance, &hdr[4], sizeof(double));
    }
    info->edge_slots = hdr[6];
  }
  PPRHIP_CHECK_HIP(hipEventSynchronize(g->ev[5]));
  info->sort_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  if (profiled) info->scan_ms = CallTimer::ms(g->ev[2], g->ev[3]);
  info->total_ms = CallTimer::ms(g->ev[0], g->ev[5]);
  return PPRHIP_OK;
}

// the first `count` positions of the last weighted sweep's profile (count <= profiled)
int wsweep_fetch(pprhip_graph* g, int32_t* order_out, uint64_t* vol_out, uint64_t* cut_out, uint64_t count) {
  if (!count || (!order_out && !vol_out && !cut_out)) return PPRHIP_OK;
  const SweepWs* w = g->sweep;
  if (order_out)
    PPRHIP_CHECK_HIP(hipMemcpyAsync(order_out, w->order, sizeof(int32_t) * count, hipMemcpyDeviceToHost, g->stream));
  if (vol_out)
    PPRHIP_CHECK_HIP(hipMemcpyAsync(vol_out, w->qvolx + 1, sizeof(uint64_t) * count, hipMemcpyDeviceToHost, g->stream));
  if (cut_out)
    PPRHIP_CHECK_HIP(hipMemcpyAsync(cut_out, w->cut, sizeof(uint64_t) * count, hipMemcpyDeviceToHost, g->stream));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  return PPRHIP_OK;
}

}  // namespace

namespace pprhip {
namespace detail {

void free_weight_quanta(GraphData* D) {
  if (D->qdeg) (void)hipFree(D->qdeg);
  D->qdeg = nullptr;
  D->q_shift = 0;
  D->q_total = D->qdeg_bytes = 0;
}

}  // namespace detail
}  // namespace pprhip

extern "C" {

int pprhip_weight_quantum(uint64_t m, const double* weights, int* shift_out) {
  static const char* fn = "pprhip_weight_quantum";
  if (!shift_out || (!weights && m)) {
    set_error("%s: bad arguments (m=%llu)", fn, (unsigned long long)m);
    return PPRHIP_ERR_INVALID;
  }
  double wmax = 0.0;
  for (uint64_t e = 0; e < m; ++e) {
    const double x = weights[e];
    if (!(std::isfinite(x) && x > 0.0)) {
      set_error("%s: edge %llu: weight %g is not finite and > 0", fn, (unsigned long long)e, x);
      return PPRHIP_ERR_INVALID;
    }
    wmax = x > wmax ? x : wmax;
  }
  *shift_out = m ? quantum_shift(wmax, m) : 0;
  return PPRHIP_OK;
}

int pprhip_weighted_sweep_cut(pprhip_graph_t* g, int normalize, uint64_t max_size, double max_vol, int32_t* order_out,
                              uint64_t* vol_q_out, uint64_t* cut_q_out, uint64_t cap, pprhip_wsweep_t* info) {
  static const char* fn = "pprhip_weighted_sweep_cut";
  PPRHIP_TRY(check_wsweep_args(fn, normalize, max_vol, order_out, vol_q_out, cut_q_out, cap, info));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  PPRHIP_TRY(wsweep_run(g, g->result_in_est ? g->est : g->reserve, normalize, max_size, max_vol, info));
  return wsweep_fetch(g, order_out, vol_q_out, cut_q_out, cap < info->profiled ? cap : info->profiled);
}

int pprhip_results_weighted_sweep_cut(pprhip_results_t* r, int i, int normalize, uint64_t max_size, double max_vol,
                                      int32_t* order_out, uint64_t* vol_q_out, uint64_t* cut_q_out, uint64_t cap,
                                      pprhip_wsweep_t* info) {
  static const char* fn = "pprhip_results_weighted_sweep_cut";
  PPRHIP_TRY(check_wsweep_args(fn, normalize, max_vol, order_out, vol_q_out, cut_q_out, cap, info));
  if (!r || i < 0 || i >= r->count) {
    set_error("%s: no result %d in the store (%d held)", fn, i, r ? r->count : 0);
    return PPRHIP_ERR_INVALID;
  }
  pprhip_graph* g = r->g;
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  PPRHIP_TRY(wsweep_run(g, r->buf + (size_t)i * g->gr->n, normalize, max_size, max_vol, info));
  return wsweep_fetch(g, order_out, vol_q_out, cut_q_out, cap < info->profiled ? cap : info->profiled);
}

int pprhip_weighted_local_cluster_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds,
                                        double alpha, double rmax, int normalize, uint64_t max_size, double max_vol,
                                        int32_t* members_out, uint64_t cap, pprhip_wsweep_t* info,
                                        pprhip_stats_t* push_stats) {
  static const char* fn = "pprhip_weighted_local_cluster_seeds";
  PPRHIP_TRY(check_wsweep_args(fn, normalize, max_vol, members_out, nullptr, nullptr, cap, info));
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_threshold(rmax, fn, "rmax"));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  // (the push checks the seed set before it touches the handle)
  PPRHIP_TRY(pprhip_weighted_forward_push_seeds(g, seeds, weights, n_seeds, alpha, rmax, nullptr, nullptr, nullptr,
                                                push_stats));
  PPRHIP_TRY(wsweep_run(g, g->reserve, normalize, max_size, max_vol, info));
  return wsweep_fetch(g, members_out, nullptr, nullptr, cap < info->best_size ? cap : info->best_size);
}

}  // extern "C"
