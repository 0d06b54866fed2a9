// seeds.cpp — queries personalized to a weighted node set (Neo4j PageRank's sourceNodes, which the reference only ever
// passes one node: Neo4j_Method.java:73-77): the caller's arrays normalized into p, p resolved for the dead-end seeds,
// the seed table in HBM, and the first frontier of a push from p (the forward push calls: forward_calls.cpp, FORA:
// fora.cpp, top-k: engine.cpp, the weighted top-k rounds: weighted_query.cpp).  DESIGN.md §2 "Seed sets" states the rule.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "engine_internal.hpp"

namespace pprhip {
namespace detail {

int seed_plan(pprhip_graph* g, const int32_t* seeds, const double* weights, int k, double alpha, const char* fn,
              SeedTable& t, int set) {
  WeightedSet p;  // distinct original ids and their normalized weights
  PPRHIP_TRY(parse_weighted_set(g->gr->n, seeds, weights, k, true, "seed", fn, set, p));
  struct E {
    int32_t v;
    double p;
  };
  std::vector<E> live, dead;
  double D = 0.0;
  for (const auto& x : p) {
    const int32_t v = g->gr->h_old2new[x.first];
    if (hdeg_out(g, v) == 0) {
      dead.push_back({v, x.second});
      D += x.second;
    } else {
      live.push_back({v, x.second});
    }
  }
  auto by_id = [](const E& a, const E& b) { return a.v < b.v; };
  std::sort(live.begin(), live.end(), by_id);
  std::sort(dead.begin(), dead.end(), by_id);
  // mass x landing on p: live seed i gets x p_i / (1 - (1 - alpha) D) as residue, dead-end seed j alpha x p_j / (...)
  // as reserve - the closed form of landing, taking alpha, and landing again at the dead-end seeds
  const double den = 1.0 - (1.0 - alpha) * D;
  t.h_id.clear();
  t.h_w.clear();
  t.h_eoff.clear();
  t.h_zin.clear();
  t.e_live = 0;
  t.max_id = -1;
  for (const E& x : live) {
    t.h_id.push_back(x.v);
    t.h_w.push_back(x.p / den);
    t.h_eoff.push_back((uint32_t)t.e_live);
    t.e_live += hdeg_out(g, x.v);
    if (hdeg_in(g, x.v) == 0) t.h_zin.push_back(x.v);
    t.max_id = std::max(t.max_id, x.v);
  }
  for (const E& x : dead) {
    t.h_id.push_back(x.v);
    t.h_w.push_back(live.empty() ? x.p : alpha * x.p / den);  // (every seed a dead end: the result is p itself)
    t.max_id = std::max(t.max_id, x.v);
  }
  t.n_live = (uint32_t)live.size();
  t.n_dead = (uint32_t)dead.size();
  t.n_zin = (uint32_t)t.h_zin.size();
  return PPRHIP_OK;
}

int seed_plan_sets(pprhip_graph* g, const int32_t* seeds, const double* weights, const uint64_t* offsets, int q,
                   double alpha, const char* fn, std::vector<SeedTable>& plans) {
  plans.clear();
  if (q < 0 || (q > 0 && !offsets)) {
    set_error("%s: bad arguments (q=%d, offsets %s)", fn, q, offsets ? "given" : "NULL");
    return PPRHIP_ERR_INVALID;
  }
  if (q == 0) return PPRHIP_OK;
  PPRHIP_TRY(check_set_offsets(offsets, q, fn));
  if (offsets[q] > 0 && !seeds) {
    set_error("%s: seeds is NULL for %llu entries", fn, (unsigned long long)offsets[q]);
    return PPRHIP_ERR_INVALID;
  }
  try {
    plans.resize((size_t)q);
    for (int i = 0; i < q; ++i) {
      const size_t o = (size_t)offsets[i];
      const int rc = seed_plan(g, seeds ? seeds + o : nullptr, weights ? weights + o : nullptr,
                               (int)(offsets[i + 1] - offsets[i]), alpha, fn, plans[(size_t)i], i);
      if (rc != PPRHIP_OK) {
        plans.clear();
        return rc;
      }
    }
  } catch (const std::bad_alloc&) {
    plans.clear();
    set_error("%s: out of host memory for the plans of %d seed sets", fn, q);
    return PPRHIP_ERR_OOM;
  }
  return PPRHIP_OK;
}

int seed_upload(pprhip_graph* g, SeedTable& plan) {
  if (!g->seeds) {
    g->seeds = new (std::nothrow) SeedTable();
    if (!g->seeds) return PPRHIP_ERR_OOM;
  }
  SeedTable& t = *g->seeds;
  const uint32_t count = plan.n_live + plan.n_dead;
  if (!t.w_node) {  // (all-zero from here on: each upload clears the entries of the set before)
    PPRHIP_TRY(alloc_dev((void**)&t.w_node, sizeof(double) * (size_t)g->gr->n));
    PPRHIP_TRY(alloc_dev((void**)&t.done, sizeof(unsigned int)));
    PPRHIP_CHECK_HIP(hipMemsetAsync(t.w_node, 0, sizeof(double) * (size_t)g->gr->n, g->stream));
    PPRHIP_CHECK_HIP(hipMemsetAsync(t.done, 0, sizeof(unsigned int), g->stream));
  }
  PPRHIP_TRY(launch_seed_clear(g, t.n_live));  // the set before's landing weights, while its ids are still in the table
  if (count > t.cap) {
    void* old[] = {t.id, t.w, t.eoff, t.zin};
    for (void* q : old)
      if (q) (void)hipFree(q);  // (hipFree waits for the work queued on them)
    t.id = nullptr;
    t.w = nullptr;
    t.eoff = nullptr;
    t.zin = nullptr;
    t.cap = 0;
    const uint32_t cap = std::max<uint32_t>(count, 1024u);
    PPRHIP_TRY(alloc_dev((void**)&t.id, sizeof(int32_t) * cap));
    PPRHIP_TRY(alloc_dev((void**)&t.w, sizeof(double) * cap));
    PPRHIP_TRY(alloc_dev((void**)&t.eoff, sizeof(uint32_t) * cap));
    PPRHIP_TRY(alloc_dev((void**)&t.zin, sizeof(int32_t) * cap));
    t.cap = cap;
  }
  // Copies from pageable memory: the runtime has taken the bytes when the call returns, so the staging vectors (kept in
  // the table until the next upload) may change at once; no wait on the stream.
  t.h_id.swap(plan.h_id);
  t.h_w.swap(plan.h_w);
  t.h_eoff.swap(plan.h_eoff);
  t.h_zin.swap(plan.h_zin);
  t.n_live = plan.n_live;
  t.n_dead = plan.n_dead;
  t.n_zin = plan.n_zin;
  t.e_live = plan.e_live;
  t.max_id = plan.max_id;
  if (count) {
    PPRHIP_CHECK_HIP(hipMemcpyAsync(t.id, t.h_id.data(), sizeof(int32_t) * count, hipMemcpyHostToDevice, g->stream));
    PPRHIP_CHECK_HIP(hipMemcpyAsync(t.w, t.h_w.data(), sizeof(double) * count, hipMemcpyHostToDevice, g->stream));
  }
  if (t.n_live)
    PPRHIP_CHECK_HIP(hipMemcpyAsync(t.eoff, t.h_eoff.data(), sizeof(uint32_t) * t.n_live, hipMemcpyHostToDevice, g->stream));
  if (t.n_zin)
    PPRHIP_CHECK_HIP(hipMemcpyAsync(t.zin, t.h_zin.data(), sizeof(int32_t) * t.n_zin, hipMemcpyHostToDevice, g->stream));
  return PPRHIP_OK;
}

// r = q on the live seeds, reserve = e on the dead-end seeds (p itself when no seed is live), the live seeds - they pop
// unconditionally - as the list fbuf
static int seed_frontier(pprhip_graph* g, int fbuf, uint32_t* nf, uint64_t* ef) {
  const SeedTable& t = *g->seeds;
  if (t.n_live + t.n_dead) PPRHIP_TRY(launch_seed_init(g, fbuf));
  *nf = t.n_live;
  *ef = t.e_live;
  return PPRHIP_OK;
}

int seed_start(pprhip_graph* g, LevelCtx& L) {
  L.dense_prepared = false;
  L.gs_dirty = false;
  return seed_frontier(g, L.fcur, &L.nf, &L.ef);
}

int seed_start(pprhip_graph* g, WLevels& L) { return seed_frontier(g, L.fcur, &L.nf, &L.ef); }

void seed_free(pprhip_graph* g) {
  if (!g->seeds) return;
  void* ptrs[] = {g->seeds->id, g->seeds->w, g->seeds->eoff, g->seeds->zin, g->seeds->w_node, g->seeds->done};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  delete g->seeds;
  g->seeds = nullptr;
  g->seed_on = false;
}

}  // namespace detail
}  // namespace pprhip

#ifdef PPRHIP_TEST_HOOKS
using namespace pprhip;
using namespace pprhip::detail;

extern "C" {

// Test hook (libpprhip_hooks.so only): the parser behind the seed sets and behind the target sets of pprhip_ppr_targets,
// without a device, as `fn` would call it: `noun` "seed" or "target", the weights divided by their sum (normalize != 0)
// or as given.  ids_out / w_out hold `count` entries; *count_out receives the distinct ids of non-zero weight.
int pprhip_hook_parse_weighted_set(uint32_t n, const int32_t* ids_in, const double* weights, int count, int normalize,
                                   const char* noun, const char* fn, int32_t* ids_out, double* w_out, int* count_out) {
  WeightedSet e;
  PPRHIP_TRY(parse_weighted_set(n, ids_in, weights, count, normalize != 0, noun, fn, -1, e));
  for (size_t i = 0; i < e.size(); ++i) {
    if (ids_out) ids_out[i] = e[i].first;
    if (w_out) w_out[i] = e[i].second;
  }
  if (count_out) *count_out = (int)e.size();
  return PPRHIP_OK;
}

// Test hook (libpprhip_hooks.so only): the argument normalization of the seed-set entry points, without a device.
// ids_out / p_out hold n_seeds entries; *count_out receives the distinct seeds of non-zero weight.
int pprhip_hook_seed_normalize(uint32_t n, const int32_t* seeds, const double* weights, int n_seeds, int32_t* ids_out,
                               double* p_out, int* count_out) {
  return pprhip_hook_parse_weighted_set(n, seeds, weights, n_seeds, 1, "seed", "pprhip_hook_seed_normalize", ids_out,
                                        p_out, count_out);
}

}  // extern "C"
#endif
