// weighted_batch.hpp — what the batched weighted forward drivers share (weighted_batch.cpp: batched weighted FORA;
// weighted_topk_batch.cpp: batched weighted top-k): a call's columns, one sparse level of a column, the shared sweep,
// the call's bring-up; the weighted top-k loop of a single query (weighted_query.cpp), which a call of one runs; and
// the dealing rule of the merged walk launch (kernels_weighted_topk_batch.hip), for host and device.
#pragma once

#include "run.hpp"

namespace pprhip {

// The dealing rule of k_w_walk_plan_multi.  counts[c]: walks of column c's plan; base_waves: the waves of a single
// walk launch (>= 1).  T = sum of counts, per = ceil(ceil(T / 64) / base_waves) * 64 (0 when T is 0); column c owns the
// ceil(counts[c] / per) consecutive waves from first[c], wave b of them the column's walks
// [(b - first[c]) * per, min(.. + per, counts[c])).  first[16] = the waves in use <= base_waves + 15.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void walk_multi_deal(const unsigned long long counts[kBatch], uint32_t base_waves, unsigned long long* per_out,
                            uint32_t first_out[kBatch + 1]) {
  unsigned long long total = 0;
#pragma unroll
  for (int c = 0; c < kBatch; ++c) total += counts[c];
  const unsigned long long waves = base_waves ? base_waves : 1u;
  const unsigned long long groups = (total + 63) / 64;
  const unsigned long long per = (groups + waves - 1) / waves * 64;
  uint32_t at = 0;
#pragma unroll
  for (int c = 0; c < kBatch; ++c) {
    first_out[c] = at;
    if (per) at += (uint32_t)((counts[c] + per - 1) / per);
  }
  first_out[kBatch] = at;
  *per_out = per;
}

namespace detail {

struct WbatQuery {  // the query a column's workspace is running
  int query = -1;  // index in the call (-1: the column is free)
  WLevels L;       // (L.prepared: the frontier is held as contributions in the column; ccur goes unused)
  PushArgs a{};
  pprhip_stats_t st;
  bool seeded = false, live = false;
  double t0 = 0.0;  // host clock at the query's begin (ms)
};

struct WbatCall {
  pprhip_graph* P = nullptr;
  BatchJob* J = nullptr;
  double alpha = 0.0, rmax = 0.0, omega = 0.0;
  unsigned long long dense_thresh = 0;
  int n_cols = kBatch;
  int next = 0;  // the call's next query
  WbatQuery q[kBatch];
};

inline pprhip_graph* slot_of(const WbatCall& C, int c) { return C.P->batch->slots[(size_t)c]; }

// ---- weighted_batch.cpp
// One sparse level of column c's query (C.q[c]: its frontier, its arguments) on its own workspace, without a read-back.
// *cell: where the level leaves the next frontier's counter.
int wbat_sparse_level(WbatCall& C, int c, const unsigned long long** cell);
// The sweep of the columns in `dense` at their own arguments, and the level bookkeeping of their queries; the counters
// arrive in the batch state's sweep_out.
int wbat_sweep(WbatCall& C, const bool* dense, int n_dense);
// bring-up and end of a batched weighted call around its driver loop `rounds(C, arg)`
int wbat_run(pprhip_graph_t* g, BatchJob& J, WbatCall& C, int (*rounds)(WbatCall&, void*), void* arg, const char* what,
             pprhip_stats_t* stats_sum);

// ---- weighted_query.cpp
// The weighted top-k loop of one query from the seed table `plan` on the handle's own workspace
// (pprhip_weighted_fora_topk / _seeds behind their checks).
int weighted_topk_drive(pprhip_graph* g, SeedTable& plan, double eps, const pprhip_fora_conf_t* conf, uint64_t seed,
                        int32_t* ids_out, double* vals_out, int cap, int* n_out, double* reserve_out,
                        pprhip_stats_t* stats);

}  // namespace detail
}  // namespace pprhip
