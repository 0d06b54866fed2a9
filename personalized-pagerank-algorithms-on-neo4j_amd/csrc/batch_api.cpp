// batch_api.cpp — the batched C entry points (sources, seed sets, top-k) over batch_run (batch.cpp), and the
// device-resident result store.
#include <cstring>
#include <new>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

// The checked arguments of the two whole-graph FORA entry points as a job: q queries from srcs, or (srcs NULL) from
// the seed sets whose plans the caller has put into J.sets.
static int fora_batch(BatchJob& J, pprhip_graph_t* g, const int32_t* srcs, int q, double eps,
                      const pprhip_fora_conf_t* conf, uint64_t seed, int n_rounds, pprhip_results_t* keep,
                      double* reserve_out, int k, int32_t* ids_out, double* vals_out, int* n_out,
                      pprhip_stats_t* per_query, pprhip_stats_t* stats_sum) {
  J.P = g;
  J.srcs = srcs;
  J.q = q;
  J.eps = eps;
  J.conf = conf;
  J.seed = seed;
  J.n_rounds = n_rounds;
  J.reserve_out = reserve_out;
  J.k = k;
  J.ids_out = ids_out;
  J.vals_out = vals_out;
  J.n_out = n_out;
  J.per_query = per_query;
  J.keep = keep;
  if (keep) keep->count = 0;
  PPRHIP_TRY(batch_run(g, J, stats_sum));
  if (keep) keep->count = q;
  return PPRHIP_OK;
}

// ... and of the two top-k entry points: query i runs with seed + i, as pprhip_fora_topk(srcs[i], ..., seed + i) or
// pprhip_fora_topk_seeds(set i, ..., seed + i) would
static int topk_batch(BatchJob& J, pprhip_graph_t* g, const int32_t* srcs, int q, int k, double eps,
                      const pprhip_fora_conf_t* conf, uint64_t seed, int32_t* ids_out, double* vals_out,
                      pprhip_stats_t* stats_sum) {
  J.P = g;
  J.kind = QueryKind::kTopk;
  J.srcs = srcs;
  J.q = q;
  J.eps = eps;
  J.conf = conf;
  J.seed = seed;
  J.k = k;
  J.ids_out = ids_out;
  J.vals_out = vals_out;
  return batch_run(g, J, stats_sum);
}

// Batched single-source FORA: up to kBatch queries in flight on kBatch workspaces of this handle.
// Every query runs the single-query algorithm unchanged (same levels, same thresholds, same walks
// for the same seed); whenever the queries in a push phase all stand at a dense level, one sweep of
// the batched kernels serves them.  All slots run on the calling thread and the handle's stream;
// with PPRHIP_BATCH_THREADS=1 (the default of the top-k entry point) every slot gets a worker
// thread and a stream of its own, so sparse levels, walks and selections of different queries
// overlap on the GPU.
int pprhip_fora_batch_single_source_resident(pprhip_graph_t* g, const int32_t* srcs, int q, double eps,
                                             const pprhip_fora_conf_t* conf, uint64_t seed, int n_rounds,
                                             pprhip_results_t* keep, double* reserve_out, int k, int32_t* ids_out,
                                             double* vals_out, int* n_out, pprhip_stats_t* per_query,
                                             pprhip_stats_t* stats_sum) {
  PPRHIP_TRY(check_positive(eps, "pprhip_fora_batch_single_source", "eps"));
  PPRHIP_TRY(check_conf(conf, "pprhip_fora_batch_single_source", false));
  PPRHIP_TRY(check_graph(g, "pprhip_fora_batch_single_source"));
  if (q < 0 || !conf || !(eps > 0.0) || n_rounds < 0 || (q > 0 && !srcs) || k < 0 ||
      (k > 0 && q > 0 && (!ids_out || !vals_out))) {
    set_error("pprhip_fora_batch_single_source: bad arguments (q=%d eps=%g n_rounds=%d k=%d)", q, eps, n_rounds, k);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_keep(keep, g, q, "pprhip_fora_batch_single_source_resident"));
  for (int i = 0; i < q; ++i) PPRHIP_TRY(check_node(g, srcs[i], "pprhip_fora_batch_single_source"));
  BatchJob J;
  return fora_batch(J, g, srcs, q, eps, conf, seed, n_rounds, keep, reserve_out, k, ids_out, vals_out, n_out, per_query,
                    stats_sum);
}

int pprhip_fora_batch_single_source(pprhip_graph_t* g, const int32_t* srcs, int q, double eps,
                                    const pprhip_fora_conf_t* conf, uint64_t seed, int n_rounds,
                                    double* reserve_out, int k, int32_t* ids_out, double* vals_out, int* n_out,
                                    pprhip_stats_t* per_query, pprhip_stats_t* stats_sum) {
  return pprhip_fora_batch_single_source_resident(g, srcs, q, eps, conf, seed, n_rounds, nullptr, reserve_out, k,
                                                  ids_out, vals_out, n_out, per_query, stats_sum);
}

// ------------------------------------------------------------------ device-resident result store
int pprhip_results_create(pprhip_graph_t* g, int capacity, pprhip_results_t** results_out) {
  PPRHIP_TRY(check_graph(g, "pprhip_results_create"));
  if (capacity < 1 || !results_out) {
    set_error("pprhip_results_create: bad arguments (capacity=%d)", capacity);
    return PPRHIP_ERR_INVALID;
  }
  pprhip_results* r = new (std::nothrow) pprhip_results();
  if (!r) return PPRHIP_ERR_OOM;
  r->g = g;
  r->device = g->gr->device;
  r->capacity = capacity;
  const int rc = alloc_dev((void**)&r->buf, sizeof(double) * (size_t)capacity * g->gr->n);
  if (rc != PPRHIP_OK) {
    delete r;
    return rc;
  }
  *results_out = r;
  return PPRHIP_OK;
}

void pprhip_results_destroy(pprhip_results_t* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->buf) (void)hipFree(r->buf);
  delete r;
}

int pprhip_results_info(const pprhip_results_t* r, int* capacity, int* count, uint32_t* n) {
  if (!r) {
    set_error("pprhip_results_info: null store");
    return PPRHIP_ERR_INVALID;
  }
  if (capacity) *capacity = r->capacity;
  if (count) *count = r->count;
  if (n) *n = r->g->gr->n;
  return PPRHIP_OK;
}

static int results_slot(pprhip_results_t* r, int i, const char* fn) {
  if (!r || i < 0 || i >= r->count) {
    set_error("%s: no result %d in the store (%d held)", fn, i, r ? r->count : 0);
    return PPRHIP_ERR_INVALID;
  }
  return check_graph(r->g, fn);
}

int pprhip_results_fetch(pprhip_results_t* r, int i, double* reserve_out) {
  PPRHIP_TRY(results_slot(r, i, "pprhip_results_fetch"));
  if (!reserve_out) {
    set_error("pprhip_results_fetch: null output");
    return PPRHIP_ERR_INVALID;
  }
  return copy_out(r->g, r->buf + (size_t)i * r->g->gr->n, reserve_out);
}

int pprhip_results_sum(pprhip_results_t* r, int i, double* sum_out) {
  PPRHIP_TRY(results_slot(r, i, "pprhip_results_sum"));
  if (!sum_out) {
    set_error("pprhip_results_sum: null output");
    return PPRHIP_ERR_INVALID;
  }
  return device_sum(r->g, r->buf + (size_t)i * r->g->gr->n, sum_out, r->g->gr->n);
}

int pprhip_fora_batch_topk(pprhip_graph_t* g, const int32_t* srcs, int q, int k, double eps, double alpha,
                           uint64_t seed, int32_t* ids_out, double* vals_out, pprhip_stats_t* stats_sum) {
  PPRHIP_TRY(check_positive(eps, "pprhip_fora_batch_topk", "eps"));
  PPRHIP_TRY(check_alpha(alpha, "pprhip_fora_batch_topk"));
  PPRHIP_TRY(check_graph(g, "pprhip_fora_batch_topk"));
  if (q < 0 || k < 1 || !(eps > 0.0) || (q > 0 && (!srcs || !ids_out || !vals_out))) {
    set_error("pprhip_fora_batch_topk: bad arguments");
    return PPRHIP_ERR_INVALID;
  }
  for (int i = 0; i < q; ++i) PPRHIP_TRY(check_node(g, srcs[i], "pprhip_fora_batch_topk"));
  pprhip_fora_conf_t conf;
  PPRHIP_TRY(pprhip_conf_fora_topk(g->gr->n, g->gr->m, k, alpha, &conf));
  BatchJob J;
  return topk_batch(J, g, srcs, q, k, eps, &conf, seed, ids_out, vals_out, stats_sum);
}

// ------------------------------------------------------------------ batched seed sets
// pprhip_fora_batch_single_source_resident / pprhip_fora_batch_topk over seed sets: query i runs as pprhip_fora_seeds
// (seed) / pprhip_fora_topk_seeds (seed + i) would run set i; every set is checked before anything runs
int pprhip_fora_batch_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, const uint64_t* offsets,
                            int q, double eps, const pprhip_fora_conf_t* conf, uint64_t seed, int n_rounds,
                            pprhip_results_t* keep, double* reserve_out, int k, int32_t* ids_out, double* vals_out,
                            int* n_out, pprhip_stats_t* per_query, pprhip_stats_t* stats_sum) {
  static const char* fn = "pprhip_fora_batch_seeds";
  PPRHIP_TRY(check_positive(eps, fn, "eps"));
  PPRHIP_TRY(check_conf(conf, fn, false));
  PPRHIP_TRY(check_graph(g, fn));
  if (q < 0 || !conf || n_rounds < 0 || k < 0 || (k > 0 && q > 0 && (!ids_out || !vals_out))) {
    set_error("%s: bad arguments (q=%d eps=%g n_rounds=%d k=%d)", fn, q, eps, n_rounds, k);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_keep(keep, g, q, fn));
  BatchJob J;
  PPRHIP_TRY(seed_plan_sets(g, seeds, weights, offsets, q, conf->alpha, fn, J.sets));
  return fora_batch(J, g, nullptr, q, eps, conf, seed, n_rounds, keep, reserve_out, k, ids_out, vals_out, n_out,
                    per_query, stats_sum);
}

int pprhip_fora_batch_topk_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights,
                                 const uint64_t* offsets, int q, int k, double eps, double alpha, uint64_t seed,
                                 int32_t* ids_out, double* vals_out, pprhip_stats_t* stats_sum) {
  static const char* fn = "pprhip_fora_batch_topk_seeds";
  PPRHIP_TRY(check_positive(eps, fn, "eps"));
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_graph(g, fn));
  if (q < 0 || k < 1 || (q > 0 && (!ids_out || !vals_out))) {
    set_error("%s: bad arguments (q=%d k=%d)", fn, q, k);
    return PPRHIP_ERR_INVALID;
  }
  pprhip_fora_conf_t conf;
  PPRHIP_TRY(pprhip_conf_fora_topk(g->gr->n, g->gr->m, k, alpha, &conf));
  BatchJob J;
  PPRHIP_TRY(seed_plan_sets(g, seeds, weights, offsets, q, conf.alpha, fn, J.sets));
  return topk_batch(J, g, nullptr, q, k, eps, &conf, seed, ids_out, vals_out, stats_sum);
}
