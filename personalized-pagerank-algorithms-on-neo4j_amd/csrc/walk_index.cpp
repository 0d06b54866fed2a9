// walk_index.cpp — the FORA+ walk index (include/pprhip.h "walk index"; DESIGN.md §2 "Walk index"): per node the
// terminals of the walks a whole-graph FORA walk phase would draw from it, built once per (alpha, seed) and kept with
// the lifted graph.  The kernels are in kernels_walk.hip (k_index_build, k_index_serve, k_mc_walk<kWalkIndexed>); the walk
// phase picks the index in launch_walk_run (device_io.cpp).  The weighted walk index (include/pprhip.h "weighted walk
// index") is the same table in a second slot of the lifted graph, filled with weighted walks (kernels_weighted.hip:
// k_w_index_build) and picked by launch_w_walk_run; the entry points of both are one set of functions here.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace pprhip {
namespace detail {

// cap(v) = ceil(d_out(v) * density) in internal order as a prefix: h_off[v] = the first position of node v, h_off[n] the
// total, which must stay below the engine's walk limit (the walk index and the call-scoped terminal cache share it)
int walk_offsets(const GraphData* D, double density, std::vector<unsigned long long>& h_off, uint64_t* total,
                 const char* fn) {
  try {
    h_off.resize((size_t)D->n + 1);
  } catch (const std::bad_alloc&) {
    set_error("%s: out of host memory", fn);
    return PPRHIP_ERR_OOM;
  }
  const double limit = (double)(1ull << kPackShift);
  unsigned long long run = 0;
  for (uint32_t v = 0; v < D->n; ++v) {
    h_off[v] = run;
    const uint32_t d = D->h_out_rp[v + 1] - D->h_out_rp[v];
    const double c = d ? std::ceil((double)d * density) : 0.0;
    if (!(c < limit) || (double)run + c >= limit) {
      set_error("%s: density = %g asks for 2^36 terminals or more (the engine's walk limit)", fn, density);
      return PPRHIP_ERR_INVALID;
    }
    run += (unsigned long long)c;
  }
  h_off[D->n] = run;
  *total = run;
  return PPRHIP_OK;
}

// ---- the table behind both (engine.hpp: TerminalTable)
// The offsets for `density`, the three device arrays, the offsets' upload and the counters' clear on `stream` (not waited
// for).  as_extra: more than a quarter of the device's free memory is refused.  Whatever fails leaves T to table_free.
static int table_alloc(TerminalTable& T, const GraphData* D, double density, int usage_cells, bool as_extra,
                       hipStream_t stream, const char* fn) {
  const size_t off_bytes = sizeof(unsigned long long) * ((size_t)D->n + 1);
  T.density = density;
  PPRHIP_TRY(walk_offsets(D, density, T.h_off, &T.total, fn));
  if (as_extra) {
    size_t free_b = 0, total_b = 0;
    PPRHIP_CHECK_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t bytes = sizeof(int32_t) * (size_t)T.total + off_bytes;
    if (bytes > free_b / 4) {
      set_error("%s: %zu bytes are more than a quarter of the device's free memory", fn, bytes);
      return PPRHIP_ERR_OOM;
    }
  }
  PPRHIP_TRY(alloc_dev((void**)&T.off, off_bytes));
  PPRHIP_TRY(alloc_dev((void**)&T.term, sizeof(int32_t) * (size_t)T.total));
  PPRHIP_TRY(alloc_dev((void**)&T.usage, usage_cells * sizeof(unsigned long long)));
  PPRHIP_CHECK_HIP(hipMemcpyAsync(T.off, T.h_off.data(), off_bytes, hipMemcpyHostToDevice, stream));
  PPRHIP_CHECK_HIP(hipMemsetAsync(T.usage, 0, usage_cells * sizeof(unsigned long long), stream));
  return PPRHIP_OK;
}

static void table_free(TerminalTable& T) {
  for (void* p : {(void*)T.off, (void*)T.term, (void*)T.usage})
    if (p) (void)hipFree(p);
}

// The cells of one node back in original ids, at most cap of them; -1 for a cell without a terminal (kWalkShareEmpty:
// the cache only).  all_streams: the cells are written on other streams than g's (the cache: the batch workspaces').
static int table_fetch_node(pprhip_graph* g, const TerminalTable& T, int32_t node, bool all_streams,
                            int32_t* terminals_out, uint64_t cap, uint64_t* count_out) {
  const int32_t v = g->gr->h_old2new[node];
  const unsigned long long o0 = T.h_off[v], cnt = T.h_off[(size_t)v + 1] - o0;
  if (count_out) *count_out = cnt;
  const uint64_t take = cnt < cap ? cnt : cap;
  if (take == 0) return PPRHIP_OK;
  if (all_streams) PPRHIP_CHECK_HIP(hipDeviceSynchronize());
  PPRHIP_CHECK_HIP(hipMemcpyAsync(terminals_out, T.term + o0, sizeof(int32_t) * take, hipMemcpyDeviceToHost, g->stream));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  for (uint64_t i = 0; i < take; ++i)
    terminals_out[i] = (uint32_t)terminals_out[i] < g->gr->n ? g->gr->h_new2old[terminals_out[i]] : -1;
  return PPRHIP_OK;
}

// the table's first two counter cells since the last reset (no table: zeros)
static int table_usage(const TerminalTable* T, uint64_t* first, uint64_t* second, int reset) {
  unsigned long long u[2] = {0ull, 0ull};
  if (T) {
    PPRHIP_CHECK_HIP(hipDeviceSynchronize());  // (the batch workspaces' streams as well)
    PPRHIP_CHECK_HIP(hipMemcpy(u, T->usage, sizeof u, hipMemcpyDeviceToHost));
    if (reset) PPRHIP_CHECK_HIP(hipMemset(T->usage, 0, sizeof u));
  }
  if (first) *first = u[0];
  if (second) *second = u[1];
  return PPRHIP_OK;
}

static uint64_t table_bytes(const TerminalTable& T, uint32_t n, int usage_cells) {  // terminals, offsets, counters
  return 4ull * T.total + 8ull * ((uint64_t)n + 1) + 8ull * (uint64_t)usage_cells;
}

static void destroy_index(WalkIndex* ix) {
  if (ix) table_free(*ix);
  delete ix;
}

void free_walk_index(WalkIndex*& slot) {
  destroy_index(slot);
  slot = nullptr;
}

// ---- the call-scoped terminal cache (engine.hpp: WalkShare)
static void free_walk_deposit(WalkDeposit& d) {
  if (d.block) (void)hipFree(d.block);
  d = WalkDeposit();
}

void free_walk_share(BatchState* B) {
  WalkShare* ws = B->share;
  if (!ws) return;
  free_walk_deposit(ws->dep);
  table_free(*ws);
  if (ws->cleared) (void)hipEventDestroy(ws->cleared);
  delete ws;
  B->share = nullptr;
}

static int walk_share_alloc(pprhip_graph* P, double density) {
  WalkShare* ws = new (std::nothrow) WalkShare();
  if (!ws) return PPRHIP_ERR_OOM;
  P->batch->share = ws;
  // (as an extra: it does not take memory the call itself may still ask for - workspaces, the fetch ring)
  PPRHIP_TRY(table_alloc(*ws, P->gr, density, 2, true, P->stream, "terminal cache"));
  PPRHIP_CHECK_HIP(hipEventCreateWithFlags(&ws->cleared, hipEventDisableTiming));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(P->stream));  // (h_off is pageable)
  return PPRHIP_OK;
}

// The deposit records of the call's walk phases (engine.hpp: WalkDeposit), decided and - on first use, or when the
// call's bound differs - allocated where the call's cache is set up, queued on P->stream in front of the cache's clear
// event.  cap: a query's walks from nodes with out-edges fit the cache's cells (the density bound), and a dead-end
// start adds at most its own entry's walks, which n covers for all that was measured; a walk beyond cap adds
// atomically, so the bound costs speed at worst.  More than a quarter of the free memory: as many records as fit.
// Whatever fails, and a graph of more than kDepMaxTiles tiles, leaves the call with its atomics and is no error.
static unsigned long long hook_number(const char* name, unsigned long long dflt) {
  const char* e = hook_env(name);
  return e && e[0] ? std::strtoull(e, nullptr, 10) : dflt;
}

static void walk_deposit_begin(pprhip_graph* P, WalkShare* ws) {
  WalkDeposit& d = ws->dep;
  d.on = false;
  const char* sw = hook_env("PPRHIP_WALK_DEPOSIT");  // test switch: atomic = the walks add at their terminals
  if (sw && sw[0] == 'a') return;
  const uint32_t n = P->gr->n;
  // test switches: a small tile (doubles, a power of two), slice, capacity and coarse bin (tiles), and the walk count
  // binning starts from
  uint32_t shift = 0;
  for (unsigned long long t = hook_number("PPRHIP_WALK_DEPOSIT_TILE", 1ull << kDepTileShift); t > 1; t >>= 1) shift++;
  if (shift < 4 || shift > kDepTileShift) shift = kDepTileShift;
  const unsigned long long slice = std::min<unsigned long long>(
      std::max<unsigned long long>(hook_number("PPRHIP_WALK_DEPOSIT_SLICE", kDepSlice), 16ull), kDepSlice);
  unsigned long long cap = std::min<unsigned long long>(ws->total + n, (1ull << 31) - 1ull);
  cap = std::min(cap, std::max<unsigned long long>(hook_number("PPRHIP_WALK_DEPOSIT_CAP", cap), 1ull));
  const unsigned long long n_tiles = ((unsigned long long)n + (1ull << shift) - 1ull) >> shift;
  if (n_tiles == 0 || n_tiles > kDepMaxTiles) return;
  // tiles per coarse bin: at most kDepMaxBin, and as many as keep the bins within kDepMaxBins
  unsigned long long bin = std::min<unsigned long long>(
      std::max<unsigned long long>(hook_number("PPRHIP_WALK_DEPOSIT_BIN", kDepBin), 1ull), kDepMaxBin);
  bin = std::max(bin, (n_tiles + kDepMaxBins - 1ull) / kDepMaxBins);
  const unsigned long long n_bins = (n_tiles + bin - 1ull) / bin;
  if (d.block && (d.want != cap || d.a.tile_shift != shift || d.a.slice != slice || d.a.bin != bin))
    free_walk_deposit(d);
  if (!d.block) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t fixed = up(4 * n_tiles) * 2 + up(4 * (n_bins + 1)) + up(16 * (n_tiles + cap / slice + 1)) +
                         up(16 * (n_bins + cap / slice + 1)) + up(4 * sizeof(unsigned long long));
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    unsigned long long fit = cap;
    if (fixed + 2 * (up(4 * fit) + up(8 * fit)) > free_b / 4) {
      if (free_b / 4 < fixed + 4096) return;
      fit = (free_b / 4 - fixed - 4096) / 24;
    }
    if (fit == 0) return;
    const size_t bytes = fixed + 2 * (up(4 * fit) + up(8 * fit));
    char* b = nullptr;
    if (alloc_dev((void**)&b, bytes) != PPRHIP_OK) {
      (void)hipGetLastError();
      return;
    }
    d.block = b;
    d.bytes = bytes;
    d.want = cap;
    DepositArgs& a = d.a;
    a.cap = fit;
    a.tile_shift = shift;
    a.n_tiles = (uint32_t)n_tiles;
    a.slice = (uint32_t)slice;
    a.items_cap = (uint32_t)(n_tiles + cap / slice + 1);
    a.bin = (uint32_t)bin;
    a.n_bins = (uint32_t)n_bins;
    a.units_cap = (uint32_t)(n_bins + cap / slice + 1);
    a.n = n;
    a.key = (uint32_t*)b;    b += up(4 * fit);
    a.bkey = (uint32_t*)b;   b += up(4 * fit);
    a.inc = (double*)b;      b += up(8 * fit);
    a.binc = (double*)b;     b += up(8 * fit);
    a.tile_cnt = (uint32_t*)b;  b += up(4 * n_tiles);
    a.tile_cur = (uint32_t*)b;  b += up(4 * n_tiles);
    a.bin_cur = (uint32_t*)b;   b += up(4 * (n_bins + 1));
    a.items = (uint4*)b;     b += up(16 * (size_t)a.items_cap);
    a.units = (uint4*)b;     b += up(16 * (size_t)a.units_cap);
    a.stat = (unsigned long long*)b;
    // the counters start at zero (k_dep_items leaves tile_cnt so); the arrays of records need no clear
    if (hipMemsetAsync(a.tile_cnt, 0, up(4 * n_tiles), P->stream) != hipSuccess ||
        hipMemsetAsync(a.stat, 0, 4 * sizeof(unsigned long long), P->stream) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipStreamSynchronize(P->stream);
      free_walk_deposit(d);
      return;
    }
  }
  d.a.min_walks = hook_number("PPRHIP_WALK_DEPOSIT_MIN", kDepMinWalks);
  d.on = true;
}

// Called where a batched whole-graph FORA call (or a stream's submission that finds the driver idle) is about to start
// its first query, with no walk kernel of the handle's slots in flight: decides whether the call's queries share
// terminals, allocates the cache on first use and clears it for the call's seed.  Whatever fails leaves the call
// without the cache and is no error.  cap(v) comes from the density bound at the threshold the queries start from
// (`rmax`: omega_i <= ceil(d_out(v) * (1 - alpha) * rmax * omega) after a push at rmax or below).
void walk_share_begin(pprhip_graph* P, int q, double alpha, double rmax, double omega, uint64_t seed) {
  BatchState* B = P->batch;
  if (B->share) B->share->on = false;
  const char* sw = hook_env("PPRHIP_WALK_SHARE");  // measurement switch: 0 = every walk is walked
  if ((sw && sw[0] == '0') || q < kWalkShareMinQueries || P->gr->widx) return;
  const double density = (1.0 - alpha) * rmax * omega * (1.0 + 0x1p-20);
  if (!(density > 0.0) || !std::isfinite(density)) return;
  if (B->share && B->share->density != density) free_walk_share(B);
  if (!B->share && walk_share_alloc(P, density) != PPRHIP_OK) {
    (void)hipGetLastError();
    free_walk_share(B);
    return;
  }
  WalkShare* ws = B->share;
  if (ws->total == 0) return;
  walk_deposit_begin(P, ws);
  if (hipMemsetAsync(ws->term, 0xFF, sizeof(int32_t) * (size_t)ws->total, P->stream) != hipSuccess ||
      hipEventRecord(ws->cleared, P->stream) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(P->stream);
    free_walk_share(B);
    return;
  }
  ws->alpha = alpha;
  ws->seed = seed;
  ws->on = true;
}

}  // namespace detail
}  // namespace pprhip

extern "C" {

int pprhip_walk_index_density(const pprhip_fora_conf_t* conf, double eps, double rmax, double* density_out) {
  static const char* fn = "pprhip_walk_index_density";
  PPRHIP_TRY(check_positive(eps, fn, "eps"));
  PPRHIP_TRY(check_conf(conf, fn, false));
  PPRHIP_TRY(check_threshold(rmax, fn, "rmax"));
  if (!conf || !density_out) {
    set_error("%s: null argument", fn);
    return PPRHIP_ERR_INVALID;
  }
  double rmax0 = 0.0, omega = 0.0;
  PPRHIP_TRY(pprhip_fora_whole_params(conf, eps, &rmax0, &omega));
  if (rmax == 0.0) rmax = rmax0;
  *density_out = (1.0 - conf->alpha) * rmax * omega * (1.0 + 0x1p-20);
  return PPRHIP_OK;
}

// ---- the two walk indexes of a lifted graph: GraphData::widx (unweighted walks) and GraphData::widx_w (weighted walks).
// The five entry points of each are these functions with the slot, the build kernel and the name messages carry.
static int index_build(pprhip_graph_t* g, bool weighted, const char* fn, double alpha, uint64_t seed, double density,
                       pprhip_stats_t* stats) {
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_positive(density, fn, "density"));
  PPRHIP_TRY(check_graph(g, fn));
  if (g->parent) {
    set_error("%s: not a graph handle", fn);
    return PPRHIP_ERR_INVALID;
  }
  if (weighted) PPRHIP_TRY(need_weights(g, fn));
  GraphData* D = g->gr;
  // (the new index is complete before the old one goes: whatever fails below frees it and leaves the handle as it was)
  std::unique_ptr<WalkIndex, void (*)(WalkIndex*)> ix(new (std::nothrow) WalkIndex(), destroy_index);
  if (!ix) return PPRHIP_ERR_OOM;
  ix->alpha = alpha;
  ix->seed = seed;
  PPRHIP_TRY(table_alloc(*ix, D, density, 3, false, g->stream, fn));
  PPRHIP_CHECK_HIP(hipEventRecord(g->ev[0], g->stream));
  PPRHIP_TRY(weighted ? launch_w_index_build(g, ix.get(), ix->usage + 2) : launch_index_build(g, ix.get(), ix->usage + 2));
  PPRHIP_CHECK_HIP(hipEventRecord(g->ev[1], g->stream));
  unsigned long long steps = 0;
  PPRHIP_CHECK_HIP(hipMemcpyAsync(&steps, ix->usage + 2, sizeof steps, hipMemcpyDeviceToHost, g->stream));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->walks = ix->total;
    stats->walk_steps = steps;
    stats->mc_ms = stats->total_ms = CallTimer::ms(g->ev[0], g->ev[1]);
    stats->mc_bytes = 12ull * steps + 4ull * ix->total + 8ull * ((uint64_t)D->n + 1);
  }
  PPRHIP_CHECK_HIP(hipDeviceSynchronize());  // nothing reads the old index any more
  WalkIndex*& slot = weighted ? D->widx_w : D->widx;
  free_walk_index(slot);
  slot = ix.release();
  return PPRHIP_OK;
}

static int index_drop(pprhip_graph_t* g, bool weighted, const char* fn) {
  PPRHIP_TRY(check_graph(g, fn));
  WalkIndex*& slot = weighted ? g->gr->widx_w : g->gr->widx;
  if (!slot) return PPRHIP_OK;
  PPRHIP_CHECK_HIP(hipDeviceSynchronize());
  free_walk_index(slot);
  return PPRHIP_OK;
}

static int index_info(const pprhip_graph_t* g, bool weighted, const char* fn, int* present, double* alpha, uint64_t* seed,
                      double* density, uint64_t* terminals, uint64_t* bytes) {
  if (!g) {
    set_error("%s: null graph handle", fn);
    return PPRHIP_ERR_INVALID;
  }
  const WalkIndex* ix = weighted ? g->gr->widx_w : g->gr->widx;
  if (present) *present = ix ? 1 : 0;
  if (alpha) *alpha = ix ? ix->alpha : 0.0;
  if (seed) *seed = ix ? ix->seed : 0;
  if (density) *density = ix ? ix->density : 0.0;
  if (terminals) *terminals = ix ? ix->total : 0;
  if (bytes) *bytes = ix ? table_bytes(*ix, g->gr->n, 3) : 0;
  return PPRHIP_OK;
}

static int index_fetch(pprhip_graph_t* g, bool weighted, const char* fn, int32_t node, int32_t* terminals_out, uint64_t cap,
                       uint64_t* count_out) {
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(check_node(g, node, fn));
  const WalkIndex* ix = weighted ? g->gr->widx_w : g->gr->widx;
  if (!ix) {
    set_error(weighted ? "%s: the handle has no weighted walk index" : "%s: the handle has no walk index", fn);
    return PPRHIP_ERR_STATE;
  }
  if (cap && !terminals_out) {
    set_error("%s: null output", fn);
    return PPRHIP_ERR_INVALID;
  }
  return table_fetch_node(g, *ix, node, false, terminals_out, cap, count_out);
}

int pprhip_walk_index_build(pprhip_graph_t* g, double alpha, uint64_t seed, double density, pprhip_stats_t* stats) {
  return index_build(g, false, "pprhip_walk_index_build", alpha, seed, density, stats);
}

int pprhip_walk_index_drop(pprhip_graph_t* g) { return index_drop(g, false, "pprhip_walk_index_drop"); }

int pprhip_walk_index_info(const pprhip_graph_t* g, int* present, double* alpha, uint64_t* seed, double* density,
                           uint64_t* terminals, uint64_t* bytes) {
  return index_info(g, false, "pprhip_walk_index_info", present, alpha, seed, density, terminals, bytes);
}

int pprhip_walk_index_fetch(pprhip_graph_t* g, int32_t node, int32_t* terminals_out, uint64_t cap, uint64_t* count_out) {
  return index_fetch(g, false, "pprhip_walk_index_fetch", node, terminals_out, cap, count_out);
}

int pprhip_walk_index_usage(pprhip_graph_t* g, uint64_t* served, uint64_t* walked, int reset) {
  PPRHIP_TRY(check_graph(g, "pprhip_walk_index_usage"));
  return table_usage(g->gr->widx, served, walked, reset);
}

int pprhip_weighted_walk_index_build(pprhip_graph_t* g, double alpha, uint64_t seed, double density,
                                     pprhip_stats_t* stats) {
  return index_build(g, true, "pprhip_weighted_walk_index_build", alpha, seed, density, stats);
}

int pprhip_weighted_walk_index_drop(pprhip_graph_t* g) { return index_drop(g, true, "pprhip_weighted_walk_index_drop"); }

int pprhip_weighted_walk_index_info(const pprhip_graph_t* g, int* present, double* alpha, uint64_t* seed, double* density,
                                    uint64_t* terminals, uint64_t* bytes) {
  return index_info(g, true, "pprhip_weighted_walk_index_info", present, alpha, seed, density, terminals, bytes);
}

int pprhip_weighted_walk_index_fetch(pprhip_graph_t* g, int32_t node, int32_t* terminals_out, uint64_t cap,
                                     uint64_t* count_out) {
  return index_fetch(g, true, "pprhip_weighted_walk_index_fetch", node, terminals_out, cap, count_out);
}

int pprhip_weighted_walk_index_usage(pprhip_graph_t* g, uint64_t* served, uint64_t* walked, int reset) {
  PPRHIP_TRY(check_graph(g, "pprhip_weighted_walk_index_usage"));
  return table_usage(g->gr->widx_w, served, walked, reset);
}

#ifdef PPRHIP_TEST_HOOKS
// Test hooks (libpprhip_hooks.so only) of the call-scoped terminal cache: whether the handle holds one and for which
// seed; the walks it served / the terminals stored since the last reset; the cells of one node (original ids, -1: not
// drawn yet), as pprhip_walk_index_fetch gives the index's.
int pprhip_hook_walk_share_info(pprhip_graph_t* g, int* present, int* on, uint64_t* seed, uint64_t* cells,
                                uint64_t* bytes) {
  PPRHIP_TRY(check_graph(g, "pprhip_hook_walk_share_info"));
  const WalkShare* ws = g->batch ? g->batch->share : nullptr;
  if (present) *present = ws ? 1 : 0;
  if (on) *on = ws && ws->on ? 1 : 0;
  if (seed) *seed = ws ? ws->seed : 0;
  if (cells) *cells = ws ? ws->total : 0;
  if (bytes) *bytes = ws ? table_bytes(*ws, g->gr->n, 2) : 0;
  return PPRHIP_OK;
}

int pprhip_hook_walk_share_usage(pprhip_graph_t* g, uint64_t* served, uint64_t* stored, int reset) {
  PPRHIP_TRY(check_graph(g, "pprhip_hook_walk_share_usage"));
  return table_usage(g->batch ? g->batch->share : nullptr, served, stored, reset);
}

int pprhip_hook_walk_share_fetch(pprhip_graph_t* g, int32_t node, int32_t* terminals_out, uint64_t cap,
                                 uint64_t* count_out) {
  static const char* fn = "pprhip_hook_walk_share_fetch";
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(check_node(g, node, fn));
  const WalkShare* ws = g->batch ? g->batch->share : nullptr;
  if (!ws || (cap && !terminals_out)) {
    set_error("%s: no terminal cache on the handle, or null output", fn);
    return PPRHIP_ERR_STATE;
  }
  return table_fetch_node(g, *ws, node, true, terminals_out, cap, count_out);
}

// ... and of the call's deposit records (engine.hpp: WalkDeposit): whether the handle holds them and the call in flight
// (or the last one) uses them, their shape, and stat_out[4] = {items of the last binned phase; since the last reset:
// binned phases, records, walks beyond the capacity}.
int pprhip_hook_walk_deposit_info(pprhip_graph_t* g, int* present, int* on, uint64_t* cap, uint32_t* tile,
                                  uint32_t* n_tiles, uint32_t* slice, uint64_t* bytes) {
  PPRHIP_TRY(check_graph(g, "pprhip_hook_walk_deposit_info"));
  const WalkShare* ws = g->batch ? g->batch->share : nullptr;
  const WalkDeposit* d = ws && ws->dep.block ? &ws->dep : nullptr;
  if (present) *present = d ? 1 : 0;
  if (on) *on = d && d->on ? 1 : 0;
  if (cap) *cap = d ? d->a.cap : 0;
  if (tile) *tile = d ? 1u << d->a.tile_shift : 0;
  if (n_tiles) *n_tiles = d ? d->a.n_tiles : 0;
  if (slice) *slice = d ? d->a.slice : 0;
  if (bytes) *bytes = d ? d->bytes : 0;
  return PPRHIP_OK;
}

int pprhip_hook_walk_deposit_usage(pprhip_graph_t* g, uint64_t* stat_out, int reset) {
  PPRHIP_TRY(check_graph(g, "pprhip_hook_walk_deposit_usage"));
  const WalkShare* ws = g->batch ? g->batch->share : nullptr;
  unsigned long long u[4] = {0ull, 0ull, 0ull, 0ull};
  if (ws && ws->dep.block) {
    PPRHIP_CHECK_HIP(hipDeviceSynchronize());  // (the walk stream as well)
    PPRHIP_CHECK_HIP(hipMemcpy(u, ws->dep.a.stat, sizeof u, hipMemcpyDeviceToHost));
    if (reset) PPRHIP_CHECK_HIP(hipMemset(ws->dep.a.stat, 0, sizeof u));
  }
  if (stat_out)
    for (int i = 0; i < 4; ++i) stat_out[i] = u[i];
  return PPRHIP_OK;
}
#endif

}  // extern "C"
