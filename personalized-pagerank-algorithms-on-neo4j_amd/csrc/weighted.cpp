// weighted.cpp — weighted relationships (include/pprhip.h "weighted relationships"): the weights on the
// lifted graph (validation, the prefix rule, the in-row copy), the level loop of every push over P(u, v) = w / W(u),
// and the weighted power method, over kernels_weighted.hip.  The level loop is plain frontier-synchronous Jacobi: one
// level per host round trip, sparse or dense by the handle's dense_frac, no Gauss-Seidel blocks, no level batches, no
// cost model.  The weighted forward push, walk-batch and FORA calls are in forward_calls.cpp, the weighted top-k rounds
// in weighted_query.cpp, the backward direction in weighted_bwd.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace {

// The prefix rule: cum of a row = the left-to-right sequential fp64 sum in row order, wsum = its last element (0 for
// an empty row).  Validation: every weight finite and > 0, every row sum finite.  cum / wsum may be null.
int weight_table(uint32_t n, uint64_t m, const uint32_t* rp, const double* w, double* cum, double* wsum, const char* fn) {
  if (rp[0] != 0 || rp[n] != m) {
    set_error("%s: out_row_ptr[0] must be 0 and out_row_ptr[n] must equal m", fn);
    return PPRHIP_ERR_INVALID;
  }
  for (uint32_t u = 0; u < n; ++u) {
    if (rp[u + 1] < rp[u] || rp[u + 1] > m) {
      set_error("%s: out_row_ptr is not ascending at node %u", fn, u);
      return PPRHIP_ERR_INVALID;
    }
    double s = 0.0;
    for (uint64_t e = rp[u]; e < rp[u + 1]; ++e) {
      const double x = w[e];
      if (!(std::isfinite(x) && x > 0.0)) {
        set_error("%s: edge %llu (out of node %u): weight %g is not finite and > 0", fn, (unsigned long long)e, u, x);
        return PPRHIP_ERR_INVALID;
      }
      s += x;
      if (cum) cum[e] = s;
    }
    if (!std::isfinite(s)) {
      set_error("%s: node %u: the sum of its out-weights is not finite", fn, u);
      return PPRHIP_ERR_INVALID;
    }
    if (wsum) wsum[u] = s;
  }
  return PPRHIP_OK;
}

size_t padded_in_edges(uint64_t m) { return ((size_t)m + kChunkPad - 1) / kChunkPad * kChunkPad + kChunkPad; }  // as in_ci

}  // namespace

namespace pprhip {
namespace detail {

int need_weights(const pprhip_graph* g, const char* fn) {
  if (!g->gr->w_bytes) {
    set_error("%s: the handle has no relationship weights (pprhip_graph_set_weights first)", fn);
    return PPRHIP_ERR_STATE;
  }
  return PPRHIP_OK;
}

int fetch_packed(pprhip_graph* g, const unsigned long long* cell, uint32_t* nf, uint64_t* ef) {
  unsigned long long pk = 0;
  PPRHIP_TRY(fetch_small(g, cell, &pk, sizeof pk));
  *nf = (uint32_t)(pk >> kPackShift);
  *ef = pk & kPackMask;
  return PPRHIP_OK;
}

// A level is dense when nodes + edges of its frontier reach dense_frac * m (the unweighted rule); the choice changes
// the order of fp64 additions and nothing else.  Backward, a dense level sweeps the out-CSR (ensure_bwd_layout).
int run_weighted_levels(pprhip_graph* g, const PushArgs& a, WLevels& L, pprhip_stats_t& st) {
  const bool bwd = a.mode == kBackward;
  const bool seeded = g->seed_on && !bwd;
  const unsigned long long dense_thresh = (unsigned long long)std::ceil(g->tun.dense_frac * (double)g->gr->m);
  const size_t nd = sizeof(double) * g->gr->n;
  unsigned long long* const list_counter = &g->ctr->hist[1];
  const uint64_t node_bytes = bwd ? 36 : 44, edge_bytes = bwd ? 44 : 36;  // of a sparse level, per list entry / edge
  auto prepare = [&](bool dense, unsigned long long* counter) {
    return bwd ? launch_wb_prepare(g, a, L.fcur, L.nf, dense, dense ? L.ccur : 0, counter)
               : launch_w_prepare(g, a, L.fcur, L.nf, dense, dense ? L.ccur : 0, L.dslot, counter);
  };
  bool first_of_phase = false;
  while (L.nf > 0) {
    if ((unsigned long long)L.nf + L.ef >= dense_thresh) {
      if (!L.prepared) {  // list form -> contributions in place
        if (bwd) PPRHIP_TRY(ensure_bwd_layout(g));
        PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[L.ccur], 0, nd, g->stream));
        PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[L.ccur ^ 1], 0, nd, g->stream));
        PPRHIP_TRY(prepare(true, nullptr));
        L.prepared = true;
        first_of_phase = true;
      }
      const uint64_t bytes = 12ull * g->gr->m + 8ull * g->gr->m + 40ull * (bwd ? g->gr->n_nz_o : g->gr->n_nz);
      ktimer().begin(PPRHIP_KERNEL_DENSE_PULL, bytes);
      PPRHIP_TRY(bwd ? launch_wb_dense_level(g, a, L.ccur, L.pslot ^ 1)
                     : launch_w_dense_level(g, a, L.ccur, L.pslot ^ 1, L.dslot));
      ktimer().end();
      // the sweep writes the contributions of the rows it applies only; a row it skips (no in-edges forward, no
      // out-edges backward) can hold one solely from the phase's seeding, so the seeded buffer is cleared right after
      // its first level has consumed it
      if (first_of_phase) PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[L.ccur], 0, nd, g->stream));
      first_of_phase = false;
      st.dense_levels++;
      st.levels++;
      st.dense_nodes += L.nf;
      st.dense_edges += L.ef;
      st.push_bytes += bytes;
      L.ccur ^= 1;
      L.dslot ^= 1;
      L.pslot ^= 1;
      PPRHIP_TRY(fetch_packed(g, &g->ctr->packed[L.pslot], &L.nf, &L.ef));
      st.enqueues += L.nf;
      continue;
    }
    // ---- a sparse level
    uint32_t nf_list = L.nf;
    uint64_t ef_list = L.ef;
    ktimer().begin(PPRHIP_KERNEL_SPARSE_PUSH, node_bytes * L.nf + edge_bytes * L.ef);
    if (L.prepared) {
      // contributions in place -> list (forward, dead-end nodes carry none: the list is recounted; it may be empty while
      // their mass still has to land on the source, so the level runs whatever the recount says)
      PPRHIP_CHECK_HIP(hipMemsetAsync(&g->ctr->hist[0], 0, 2 * sizeof(unsigned long long), g->stream));
      PPRHIP_TRY(launch_compact_prepared(g, L.ccur, L.fcur, &g->ctr->hist[0], bwd));
      PPRHIP_TRY(fetch_packed(g, &g->ctr->hist[0], &nf_list, &ef_list));
      L.prepared = false;
    } else {
      PPRHIP_TRY(prepare(false, list_counter));
    }
    // a seeded push (SeedScope; a.src is -1): the level's dead-end mass lands on p here, and launch_w_push finds the
    // cell empty
    if (seeded) PPRHIP_TRY(launch_wq_land_sparse(g, a, L.fcur, L.dslot, list_counter));
    PPRHIP_TRY(bwd ? launch_wb_push(g, a, L.fcur, nf_list, ef_list, list_counter)
                   : launch_w_push(g, a, L.fcur, nf_list, ef_list, L.dslot, list_counter));
    ktimer().end();
    st.pops += L.nf;
    st.edge_pushes += L.ef;
    st.levels++;
    st.push_bytes += node_bytes * L.nf + edge_bytes * L.ef;
    L.fcur ^= 1;
    PPRHIP_TRY(fetch_packed(g, list_counter, &L.nf, &L.ef));
    st.enqueues += L.nf;
  }
  return PPRHIP_OK;
}

void free_weights(GraphData* D) {
  if (D->widx_w) {  // built from these weights: it goes before they change (its readers are the handle's weighted calls)
    (void)hipDeviceSynchronize();
    free_walk_index(D->widx_w);
  }
  void* ptrs[] = {D->out_w, D->out_cum, D->wsum, D->in_w, D->wsurvival};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  D->out_w = D->out_cum = D->wsum = D->in_w = D->wsurvival = nullptr;
  D->wsurvival_alpha = 0.0;
  D->w_bytes = 0;
  free_weighted_in_rec(D);
  free_weight_quanta(D);
}

void free_weighted_in_rec(GraphData* D) {
  if (D->in_wrec) (void)hipFree(D->in_wrec);
  D->in_wrec = nullptr;
  D->in_wrec_bytes = 0;
}

}  // namespace detail
}  // namespace pprhip

namespace {

// The host half of pprhip_graph_set_weights: the caller's weights validated, then the four arrays in internal order.
// in_w: the weights of every in-row, aligned with in_ci.  The out-rows are walked in internal order, which lists the
// in-edges of every row by ascending source; where the lifted in-row is in another order (the caller's in-adjacency
// decides that), its positions are matched to that list by source - parallel relationships in any assignment, which
// gives the row the multiset of its edges' weights.
int build_weight_arrays(pprhip_graph* g, const double* weights, std::vector<double>& out_w, std::vector<double>& out_cum,
                        std::vector<double>& wsum, std::vector<double>& in_w) {
  const GraphData* D = g->gr;
  const uint32_t n = D->n;
  const uint64_t m = D->m;
  const char* fn = "pprhip_graph_set_weights";
  // the caller's row pointers, from the lifted degrees
  std::vector<uint32_t> crp((size_t)n + 1, 0);
  for (uint32_t o = 0; o < n; ++o) {
    const int32_t v = D->h_old2new[o];
    crp[o + 1] = crp[o] + (D->h_out_rp[v + 1] - D->h_out_rp[v]);
  }
  std::vector<double> ccum((size_t)m), cws((size_t)n);
  PPRHIP_TRY(weight_table(n, m, crp.data(), weights, ccum.data(), cws.data(), fn));
  out_w.resize((size_t)m);
  out_cum.resize((size_t)m);
  wsum.resize((size_t)n);
  for (uint32_t v = 0; v < n; ++v) {  // rows move, the order inside a row is kept (lift.cpp: relabel_csr)
    const int32_t o = D->h_new2old[v];
    const uint32_t d = D->h_out_rp[v + 1] - D->h_out_rp[v];
    std::copy(weights + crp[o], weights + crp[o] + d, out_w.begin() + D->h_out_rp[v]);
    std::copy(ccum.begin() + crp[o], ccum.begin() + crp[o] + d, out_cum.begin() + D->h_out_rp[v]);
    wsum[v] = cws[o];
  }
  ccum = std::vector<double>();
  in_w.assign(padded_in_edges(m), 0.0);
  if (m == 0) return PPRHIP_OK;
  std::vector<int32_t> oci((size_t)m), ici((size_t)m), ts((size_t)m);
  PPRHIP_CHECK_HIP(hipMemcpy(oci.data(), D->out_ci, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
  PPRHIP_CHECK_HIP(hipMemcpy(ici.data(), D->in_ci, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
  std::vector<uint32_t> cur(D->h_in_rp.begin(), D->h_in_rp.begin() + n);
  for (uint32_t u = 0; u < n; ++u)
    for (uint32_t e = D->h_out_rp[u]; e < D->h_out_rp[u + 1]; ++e) {
      const uint32_t p = cur[oci[e]]++;
      ts[p] = (int32_t)u;
      in_w[p] = out_w[e];
    }
  std::vector<uint32_t> order;
  std::vector<double> tmp;
  for (uint32_t v = 0; v < n; ++v) {
    const uint32_t b = D->h_in_rp[v], e = D->h_in_rp[v + 1];
    if (std::equal(ts.begin() + b, ts.begin() + e, ici.begin() + b)) continue;
    order.resize(e - b);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ici[b + x] < ici[b + y]; });
    tmp.assign(in_w.begin() + b, in_w.begin() + e);
    for (uint32_t k = 0; k < e - b; ++k) {
      if (ici[b + order[k]] != ts[b + k]) {
        set_error("%s: node %d: the lifted in-row does not hold the sources of its relationships", fn, D->h_new2old[v]);
        return PPRHIP_ERR_STATE;
      }
      in_w[b + order[k]] = tmp[k];
    }
  }
  return PPRHIP_OK;
}

int upload_f64(double** dst, const std::vector<double>& src) {
  PPRHIP_TRY(alloc_dev((void**)dst, sizeof(double) * src.size()));
  if (!src.empty()) PPRHIP_CHECK_HIP(hipMemcpy(*dst, src.data(), sizeof(double) * src.size(), hipMemcpyHostToDevice));
  return PPRHIP_OK;
}

}  // namespace

extern "C" {

int pprhip_weight_table_host(uint32_t n, uint64_t m, const uint32_t* out_row_ptr, const double* weights, double* cum_out,
                             double* wsum_out) {
  if (n == 0 || !out_row_ptr || (!weights && m)) {
    set_error("pprhip_weight_table_host: bad arguments (n=%u m=%llu)", n, (unsigned long long)m);
    return PPRHIP_ERR_INVALID;
  }
  return weight_table(n, m, out_row_ptr, weights, cum_out, wsum_out, "pprhip_weight_table_host");
}

int pprhip_graph_set_weights(pprhip_graph_t* g, const double* weights) {
  PPRHIP_TRY(check_graph(g, "pprhip_graph_set_weights"));
  GraphData* D = g->gr;
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  if (!weights) {
    free_weights(D);
    return PPRHIP_OK;
  }
  double *d_ow = nullptr, *d_oc = nullptr, *d_ws = nullptr, *d_iw = nullptr;
  auto fail = [&](int rc) {
    void* ptrs[] = {d_ow, d_oc, d_ws, d_iw};
    for (void* p : ptrs)
      if (p) (void)hipFree(p);
    return rc;
  };
  try {
    std::vector<double> out_w, out_cum, wsum, in_w;
    PPRHIP_TRY(build_weight_arrays(g, weights, out_w, out_cum, wsum, in_w));
    int rc = PPRHIP_OK;
    if ((rc = upload_f64(&d_ow, out_w)) || (rc = upload_f64(&d_oc, out_cum)) || (rc = upload_f64(&d_ws, wsum)) ||
        (rc = upload_f64(&d_iw, in_w)))
      return fail(rc);
    free_weights(D);  // a second call replaces the first
    D->out_w = d_ow;
    D->out_cum = d_oc;
    D->wsum = d_ws;
    D->in_w = d_iw;
    D->w_bytes = sizeof(double) * (uint64_t)(out_w.size() + out_cum.size() + wsum.size() + in_w.size());
  } catch (const std::bad_alloc&) {
    set_error("pprhip_graph_set_weights: out of host memory");
    return fail(PPRHIP_ERR_OOM);
  }
  return PPRHIP_OK;
}

int pprhip_weights_info(const pprhip_graph_t* g, int* present, uint64_t* bytes) {
  if (!g) {
    set_error("pprhip_weights_info: null graph handle");
    return PPRHIP_ERR_INVALID;
  }
  if (present) *present = g->gr->w_bytes ? 1 : 0;
  // (the weighted All-Pair records and the weighted sweep's qdeg once they exist)
  if (bytes) *bytes = g->gr->w_bytes + g->gr->in_wrec_bytes + g->gr->qdeg_bytes;
  return PPRHIP_OK;
}

int pprhip_weighted_power_method(pprhip_graph_t* g, int32_t src, double alpha, int iters, double* reserve_out,
                                 pprhip_stats_t* stats) {
  const char* fn = "pprhip_weighted_power_method";
  PPRHIP_TRY(check_alpha(alpha, fn));
  if (iters < 0) {
    set_error("%s: iters = %d must be >= 0", fn, iters);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(check_graph(g, fn));
  PPRHIP_TRY(need_weights(g, fn));
  PPRHIP_TRY(check_node(g, src, fn));
  src = g->gr->h_old2new[src];  // internal id
  pprhip_stats_t st;
  std::memset(&st, 0, sizeof st);
  g->topk_active = false;
  PPRHIP_TRY(reset_query_state(g, false, src));
  CallTimer tm(g);
  if (iters > 0) {
    // iteration 1 with residue = {s: 1}: the source pops (reserve += alpha, c = (1 - alpha) / W, or the dead-end cell);
    // every iteration after it is one dense level in which every node with mass pops
    const size_t nd = sizeof(double) * g->gr->n;
    const PushArgs a{alpha, 0.0, 0.0, src, kPower};
    int cc = 0, ds = 0, ps = 0;
    PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[0], 0, nd, g->stream));
    PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[1], 0, nd, g->stream));
    PPRHIP_TRY(launch_set_f64(g, g->residue, (uint32_t)src, 1.0));
    PPRHIP_TRY(launch_seed_one(g, 0, src));
    PPRHIP_TRY(launch_w_prepare(g, a, 0, 1u, true, cc, ds, nullptr));
    const uint64_t bytes = 20ull * g->gr->m + 40ull * g->gr->n_nz;
    for (int it = 1; it < iters; ++it) {
      ktimer().begin(PPRHIP_KERNEL_DENSE_PULL, bytes);
      PPRHIP_TRY(launch_w_dense_level(g, a, cc, ps ^ 1, ds));
      ktimer().end();
      if (it == 1) PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[cc], 0, nd, g->stream));  // (run_weighted_levels)
      cc ^= 1;
      ds ^= 1;
      ps ^= 1;
      st.dense_levels++;
      st.levels++;
      st.push_bytes += bytes;
    }
  }
  PPRHIP_TRY(read_dead_pops(g, st));
  tm.mark(1);
  tm.finish(st);
  st.push_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  st.rounds = (uint32_t)iters;
  PPRHIP_TRY(copy_out(g, g->reserve, reserve_out));
  if (stats) *stats = st;
  return PPRHIP_OK;
}

}  // extern "C"
