// sparse.cpp — sparse results: the drivers of pprhip_get_reserve_sparse, pprhip_get_residue_sparse,
// pprhip_results_fetch_sparse and pprhip_results_fetch_sparse_all (DESIGN.md §2 "Sparse results").  It owns the handle's
// sparse workspace and sequences the steps of kernels_compact.hip on the handle's stream: tile counts, their scan, the
// scatter, for by-value the sorts.  The host waits once, for the count (the buffers and the library sorts take their
// size from it), then copies min(cap, count) entries.  The argument checks and the cap arithmetic (sparse_args.hpp)
// need no device.
#include <cstring>

#include "engine_internal.hpp"
#include "sparse_args.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace pprhip {
namespace detail {

static void free_group(void** ptrs, int count) {
  for (int i = 0; i < count; ++i) {
    if (ptrs[i]) (void)hipFree(ptrs[i]);
  }
}

void free_sparse(pprhip_graph* g) {
  SparseWs* w = g->sparse;
  if (!w) return;
  void* ptrs[] = {w->cnt, w->base, w->offs, w->val[0], w->val[1], w->id, w->pk[0], w->pk[1], w->tmp};
  free_group(ptrs, (int)(sizeof ptrs / sizeof ptrs[0]));
  delete w;
  g->sparse = nullptr;
}

// Each group holds at least `need` items afterwards: one too small is freed and allocated again with room to spare.
// An allocation that fails leaves no partial workspace behind (free_sparse), as ensure_sweep does.
static int ensure_tiles(pprhip_graph* g, size_t tiles, size_t rows) {
  if (!g->sparse && !(g->sparse = new (std::nothrow) SparseWs())) return PPRHIP_ERR_OOM;
  SparseWs* w = g->sparse;
  int rc = PPRHIP_OK;
  if (tiles > w->tile_cap) {
    void* old[] = {w->cnt, w->base};
    free_group(old, 2);
    w->cnt = w->base = nullptr;
    w->tile_cap = 0;
    if (!(rc = alloc_dev((void**)&w->cnt, sizeof(unsigned long long) * (tiles + 1))) &&
        !(rc = alloc_dev((void**)&w->base, sizeof(unsigned long long) * (tiles + 1))))
      w->tile_cap = tiles;
  }
  if (!rc && rows + 1 > w->offs_cap) {
    if (w->offs) (void)hipFree(w->offs);
    w->offs = nullptr;
    w->offs_cap = 0;
    if (!(rc = alloc_dev((void**)&w->offs, sizeof(unsigned long long) * (rows + 1)))) w->offs_cap = rows + 1;
  }
  if (rc) free_sparse(g);
  return rc;
}

static int ensure_entries(pprhip_graph* g, size_t entries, bool sorted) {
  SparseWs* w = g->sparse;
  int rc = PPRHIP_OK;
  if (entries > w->ent_cap) {
    void* old[] = {w->val[0], w->id};
    free_group(old, 2);
    w->val[0] = nullptr;
    w->id = nullptr;
    w->ent_cap = 0;
    const size_t want = sparse_grown(entries);
    if (!(rc = alloc_dev((void**)&w->val[0], sizeof(unsigned long long) * want)) &&
        !(rc = alloc_dev((void**)&w->id, sizeof(uint32_t) * want)))
      w->ent_cap = want;
  }
  if (!rc && sorted && entries > w->sort_cap) {
    void* old[] = {w->val[1], w->pk[0], w->pk[1]};
    free_group(old, 3);
    w->val[1] = w->pk[0] = w->pk[1] = nullptr;
    w->sort_cap = 0;
    const size_t want = sparse_grown(entries);
    if (!(rc = alloc_dev((void**)&w->val[1], sizeof(unsigned long long) * want)) &&
        !(rc = alloc_dev((void**)&w->pk[0], sizeof(unsigned long long) * want)) &&
        !(rc = alloc_dev((void**)&w->pk[1], sizeof(unsigned long long) * want)))
      w->sort_cap = want;
  }
  if (rc) free_sparse(g);
  return rc;
}

// The sparse form of `rows` vectors of n doubles at x (internal order, HBM): the total to *total_out, the CSR offsets
// (rows + 1 words) to offsets_out when given, the first min(cap, total) entries to ids_out / vals_out.
static int sparse_run(pprhip_graph* g, const double* x, uint32_t rows, double threshold, int order, uint64_t* offsets_out,
                      int32_t* ids_out, double* vals_out, uint64_t cap, uint64_t* total_out) {
  const size_t tiles = (size_t)((g->gr->n + kCompactTile - 1u) / kCompactTile) * rows;
  PPRHIP_TRY(ensure_tiles(g, tiles, rows));
  SparseWs* w = g->sparse;
  PPRHIP_TRY(launch_compact_count(g, w, x, rows, threshold));
  unsigned long long total = 0;
  PPRHIP_TRY(fetch_small(g, w->offs + rows, &total, sizeof total));
  if (total > (unsigned long long)g->gr->n * rows) {
    set_error("sparse results: %llu entries of %u vectors of %u", total, rows, g->gr->n);
    return PPRHIP_ERR_STATE;
  }
  *total_out = total;
  const uint64_t take = sparse_take(cap, total, ids_out || vals_out);
  if (take) {
    const bool by_value = order == PPRHIP_SPARSE_BY_VALUE;
    PPRHIP_TRY(ensure_entries(g, (size_t)total, by_value));
    w = g->sparse;
    PPRHIP_TRY(launch_compact_scatter(g, w, x, rows, threshold, by_value));
    if (by_value) PPRHIP_TRY(launch_compact_sort(g, w, total, rows));
    if (ids_out)
      PPRHIP_CHECK_HIP(hipMemcpyAsync(ids_out, w->id, sizeof(int32_t) * take, hipMemcpyDeviceToHost, g->stream));
    if (vals_out)
      PPRHIP_CHECK_HIP(hipMemcpyAsync(vals_out, w->val_out, sizeof(double) * take, hipMemcpyDeviceToHost, g->stream));
  }
  if (offsets_out)
    PPRHIP_CHECK_HIP(hipMemcpyAsync(offsets_out, w->offs, sizeof(uint64_t) * ((size_t)rows + 1), hipMemcpyDeviceToHost,
                                    g->stream));
  if (take || offsets_out) PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip

extern "C" {

int pprhip_get_reserve_sparse(pprhip_graph_t* g, double threshold, int order, int32_t* ids_out, double* vals_out,
                              uint64_t cap, uint64_t* count_out) {
  static const char* fn = "pprhip_get_reserve_sparse";
  PPRHIP_TRY(sparse_check_args(fn, threshold, order, ids_out, vals_out, cap, count_out, true));
  PPRHIP_TRY(check_graph(g, fn));
  return sparse_run(g, g->result_in_est ? g->est : g->reserve, 1, threshold, order, nullptr, ids_out, vals_out, cap,
                    count_out);
}

int pprhip_get_residue_sparse(pprhip_graph_t* g, double threshold, int order, int32_t* ids_out, double* vals_out,
                              uint64_t cap, uint64_t* count_out) {
  static const char* fn = "pprhip_get_residue_sparse";
  PPRHIP_TRY(sparse_check_args(fn, threshold, order, ids_out, vals_out, cap, count_out, true));
  PPRHIP_TRY(check_graph(g, fn));
  return sparse_run(g, g->residue, 1, threshold, order, nullptr, ids_out, vals_out, cap, count_out);
}

int pprhip_results_fetch_sparse(pprhip_results_t* r, int i, double threshold, int order, int32_t* ids_out,
                                double* vals_out, uint64_t cap, uint64_t* count_out) {
  static const char* fn = "pprhip_results_fetch_sparse";
  PPRHIP_TRY(sparse_check_args(fn, threshold, order, ids_out, vals_out, cap, count_out, true));
  if (!r || i < 0 || i >= r->count) {
    set_error("%s: no result %d in the store (%d held)", fn, i, r ? r->count : 0);
    return PPRHIP_ERR_INVALID;
  }
  pprhip_graph* g = r->g;
  PPRHIP_TRY(check_graph(g, fn));
  return sparse_run(g, r->buf + (size_t)i * g->gr->n, 1, threshold, order, nullptr, ids_out, vals_out, cap, count_out);
}

int pprhip_results_fetch_sparse_all(pprhip_results_t* r, double threshold, int order, uint64_t* offsets_out,
                                    int32_t* ids_out, double* vals_out, uint64_t cap, uint64_t* total_out) {
  static const char* fn = "pprhip_results_fetch_sparse_all";
  PPRHIP_TRY(sparse_check_args(fn, threshold, order, ids_out, vals_out, cap, total_out, offsets_out != nullptr));
  if (!r) {
    set_error("%s: null store", fn);
    return PPRHIP_ERR_INVALID;
  }
  pprhip_graph* g = r->g;
  PPRHIP_TRY(check_graph(g, fn));
  if (r->count <= 0) {  // an empty store: one offset, no entry
    offsets_out[0] = 0;
    *total_out = 0;
    return PPRHIP_OK;
  }
  return sparse_run(g, r->buf, (uint32_t)r->count, threshold, order, offsets_out, ids_out, vals_out, cap, total_out);
}

}  // extern "C"
