// sweep.cpp — local clustering: the sweep-cut driver (pprhip_sweep_cut, pprhip_results_sweep_cut,
// pprhip_local_cluster_seeds; DESIGN.md §2 "Sweep cut").  It owns the handle's sweep workspace and sequences the steps
// of kernels_sweep.hip on the handle's stream: support, order, rank table and volume, the edge scan, the best prefix.
// The host waits twice: for the support's size (the library sorts take their size on the host) and for the header.
#include <cmath>
#include <cstring>
#include <limits>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace pprhip {
namespace detail {

void free_sweep(pprhip_graph* g) {
  SweepWs* w = g->sweep;
  if (!w) return;
  void* ptrs[] = {w->key[0], w->key[1], w->id[0], w->id[1], w->rank, w->rec, w->deg, w->volx, w->tile_node, w->delta,
                  w->cut, w->part_phi, w->part_idx, w->hdr, w->tmp, w->qvolx};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete w;
  g->sweep = nullptr;
}

int ensure_sweep(pprhip_graph* g) {
  if (g->sweep) return PPRHIP_OK;
  SweepWs* w = g->sweep = new (std::nothrow) SweepWs();
  if (!w) return PPRHIP_ERR_OOM;
  const size_t n = g->gr->n;
  // (weighted_sweep.cpp also keeps the one-off list of hub rows here, two words per row of kQdegHubRow entries or more:
  // ensure_quanta checks that this capacity holds it)
  w->tile_cap = (size_t)((2 * g->gr->m + kSweepTile - 1) / kSweepTile) + 2;
  int rc = PPRHIP_OK;
  for (int i = 0; i < 2 && !rc; ++i) {
    if ((rc = alloc_dev((void**)&w->key[i], sizeof(unsigned long long) * n))) break;
    rc = alloc_dev((void**)&w->id[i], sizeof(uint32_t) * n);
  }
  if (rc || (rc = alloc_dev((void**)&w->rank, sizeof(uint32_t) * n)) || (rc = alloc_dev((void**)&w->rec, sizeof(uint4) * n)) ||
      (rc = alloc_dev((void**)&w->deg, sizeof(unsigned long long) * n)) ||
      (rc = alloc_dev((void**)&w->volx, sizeof(unsigned long long) * (n + 1))) ||
      (rc = alloc_dev((void**)&w->tile_node, sizeof(uint32_t) * w->tile_cap)) ||
      (rc = alloc_dev((void**)&w->delta, sizeof(long long) * n)) ||
      (rc = alloc_dev((void**)&w->cut, sizeof(unsigned long long) * n)) ||
      (rc = alloc_dev((void**)&w->part_phi, sizeof(double) * kSweepBestBlocks)) ||
      (rc = alloc_dev((void**)&w->part_idx, sizeof(unsigned long long) * kSweepBestBlocks)) ||
      (rc = alloc_dev((void**)&w->hdr, sizeof(unsigned long long) * kSweepHdrWords))) {
    free_sweep(g);  // e.g. out of memory half-way: leave no partial workspace behind
    return rc;
  }
  return PPRHIP_OK;
}

// "Parameter ranges" and buffers, before the handle is looked at
static int check_sweep_args(const char* fn, int normalize, const void* a, const void* b, const void* c, uint64_t cap,
                            const pprhip_sweep_t* info) {
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
  return PPRHIP_OK;
}

// the sweep over x (internal order, n doubles in HBM); order / vol / cut stay in the workspace (sweep_fetch)
static int sweep_run(pprhip_graph* g, const double* x, int normalize, uint64_t max_size, uint64_t max_vol,
                     pprhip_sweep_t* info) {
  std::memset(info, 0, sizeof *info);
  info->best_conductance = std::numeric_limits<double>::infinity();
  info->total_vol = 2ull * g->gr->m;
  PPRHIP_TRY(ensure_sweep(g));
  SweepWs* w = g->sweep;
  PPRHIP_CHECK_HIP(hipEventRecord(g->ev[0], g->stream));
  PPRHIP_TRY(launch_sweep_support(g, w, x, normalize));
  unsigned long long support = 0;
  PPRHIP_TRY(fetch_small(g, w->hdr, &support, sizeof support));
  if (support > g->gr->n) {
    set_error("sweep: %llu ranked nodes of %u", support, g->gr->n);
    return PPRHIP_ERR_STATE;
  }
  info->support = support;
  const uint32_t profiled = (uint32_t)(max_size > 0 && max_size < support ? max_size : support);
  info->profiled = profiled;
  if (support) PPRHIP_TRY(launch_sweep_sort(g, w, (uint32_t)support));
  PPRHIP_CHECK_HIP(hipEventRecord(g->ev[1], g->stream));
  if (profiled) {
    PPRHIP_TRY(launch_sweep_rank(g, w, profiled));
    PPRHIP_TRY(launch_sweep_edges(g, w, profiled, g->ev[2], g->ev[3]));
    PPRHIP_TRY(launch_sweep_best(g, w, profiled, max_vol));
  }
  PPRHIP_CHECK_HIP(hipEventRecord(g->ev[5], g->stream));
  if (profiled) {
    unsigned long long hdr[kSweepHdrWords];
    PPRHIP_TRY(fetch_small(g, w->hdr, hdr, sizeof hdr));
    info->best_size = hdr[1];
    info->best_cut = hdr[2];
    info->best_vol = hdr[3];
    std::memcpy(&info->best_conductance, &hdr[4], sizeof(double));
    info->edge_slots = hdr[5];
  }
  PPRHIP_CHECK_HIP(hipEventSynchronize(g->ev[5]));
  info->sort_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  if (profiled) info->scan_ms = CallTimer::ms(g->ev[2], g->ev[3]);
  info->total_ms = CallTimer::ms(g->ev[0], g->ev[5]);
  return PPRHIP_OK;
}

// the first `count` positions of the last sweep's profile (count <= profiled)
static int sweep_fetch(pprhip_graph* g, int32_t* order_out, uint64_t* vol_out, uint64_t* cut_out, uint64_t count) {
  if (!count || (!order_out && !vol_out && !cut_out)) return PPRHIP_OK;
  const SweepWs* w = g->sweep;
  if (order_out)
    PPRHIP_CHECK_HIP(hipMemcpyAsync(order_out, w->order, sizeof(int32_t) * count, hipMemcpyDeviceToHost, g->stream));
  if (vol_out)
    PPRHIP_CHECK_HIP(hipMemcpyAsync(vol_out, w->volx + 1, sizeof(uint64_t) * count, hipMemcpyDeviceToHost, g->stream));
  if (cut_out)
    PPRHIP_CHECK_HIP(hipMemcpyAsync(cut_out, w->cut, sizeof(uint64_t) * count, hipMemcpyDeviceToHost, g->stream));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip

extern "C" {

int pprhip_sweep_cut(pprhip_graph_t* g, int normalize, uint64_t max_size, uint64_t max_vol, int32_t* order_out,
                     uint64_t* vol_out, uint64_t* cut_out, uint64_t cap, pprhip_sweep_t* info) {
  static const char* fn = "pprhip_sweep_cut";
  PPRHIP_TRY(check_sweep_args(fn, normalize, order_out, vol_out, cut_out, cap, info));
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(sweep_run(g, g->result_in_est ? g->est : g->reserve, normalize, max_size, max_vol, info));
  return sweep_fetch(g, order_out, vol_out, cut_out, cap < info->profiled ? cap : info->profiled);
}

int pprhip_results_sweep_cut(pprhip_results_t* r, int i, int normalize, uint64_t max_size, uint64_t max_vol,
                             int32_t* order_out, uint64_t* vol_out, uint64_t* cut_out, uint64_t cap,
                             pprhip_sweep_t* info) {
  static const char* fn = "pprhip_results_sweep_cut";
  PPRHIP_TRY(check_sweep_args(fn, normalize, order_out, vol_out, cut_out, cap, info));
  if (!r || i < 0 || i >= r->count) {
    set_error("%s: no result %d in the store (%d held)", fn, i, r ? r->count : 0);
    return PPRHIP_ERR_INVALID;
  }
  pprhip_graph* g = r->g;
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(sweep_run(g, r->buf + (size_t)i * g->gr->n, normalize, max_size, max_vol, info));
  return sweep_fetch(g, order_out, vol_out, cut_out, cap < info->profiled ? cap : info->profiled);
}

int pprhip_local_cluster_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds, double alpha,
                               double rmax, int normalize, uint64_t max_size, uint64_t max_vol, int32_t* members_out,
                               uint64_t cap, pprhip_sweep_t* info, pprhip_stats_t* push_stats) {
  static const char* fn = "pprhip_local_cluster_seeds";
  PPRHIP_TRY(check_sweep_args(fn, normalize, members_out, nullptr, nullptr, cap, info));
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_threshold(rmax, fn, "rmax"));
  PPRHIP_TRY(check_graph(g, fn));
  // (the push checks the seed set before it touches the handle)
  PPRHIP_TRY(pprhip_forward_push_seeds(g, seeds, weights, n_seeds, alpha, rmax, nullptr, nullptr, nullptr, push_stats));
  PPRHIP_TRY(sweep_run(g, g->reserve, normalize, max_size, max_vol, info));
  return sweep_fetch(g, members_out, nullptr, nullptr, cap < info->best_size ? cap : info->best_size);
}

}  // extern "C"
