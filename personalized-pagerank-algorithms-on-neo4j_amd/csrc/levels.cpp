// levels.cpp — the level loop (run_levels: batches of dense and of sparse levels until the frontier is empty) and
// what only it uses: the packed frontier counters, the level cost model, the Gauss-Seidel block plan and the sliced
// layout's windows, and the scans that seed a frontier.  Read-backs and scopes: device_io.cpp; workspaces and
// layouts: graph.cpp; the kernels: kernels_push.hip, kernels_dense.hip, kernels_frontier.hip (shared declarations:
// engine_internal.hpp).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <mutex>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace pprhip {
namespace detail {

int read_packed(pprhip_graph* g, int slot, uint32_t* nf, uint64_t* ef) {
  PPRHIP_TRY(fetch_small(g, &g->ctr->packed[slot], &g->h_ctr->packed[slot], sizeof(unsigned long long)));
  const unsigned long long pk = g->h_ctr->packed[slot];
  *nf = (uint32_t)(pk >> kPackShift);
  *ef = pk & kPackMask;
  return PPRHIP_OK;
}

int zero_packed(pprhip_graph* g, int slot) {
  PPRHIP_CHECK_HIP(hipMemsetAsync(&g->ctr->packed[slot], 0, sizeof(unsigned long long), g->stream));
  return PPRHIP_OK;
}

int write_packed(pprhip_graph* g, int slot, uint32_t nf, uint64_t ef) {
  g->h_ctr->packed[slot] = ((unsigned long long)nf << kPackShift) | ef;
  PPRHIP_CHECK_HIP(hipMemcpyAsync(&g->ctr->packed[slot], &g->h_ctr->packed[slot], sizeof(unsigned long long),
                                  hipMemcpyHostToDevice, g->stream));
  return PPRHIP_OK;
}

// modelled cost of a dense sweep (level_cost's dense branch): also what a sweep costs that only runs because the
// contribution array has to be flushed
double dense_sweep_cost(const pprhip_graph* g) {
  const pprhip_tuning_t& t = g->tun;
  return t.c_level_ns + t.c_dense_edge_ns * (double)g->gr->m + t.c_dense_node_ns * (double)g->gr->n;
}

// level cost model; the test twin evaluates the same expression
double level_cost(const pprhip_graph* g, uint64_t nf, uint64_t ef, bool* dense) {
  const pprhip_tuning_t& t = g->tun;
  const bool d = (double)(ef + nf) >= t.dense_frac * (double)g->gr->m;
  *dense = d;
  if (d) return dense_sweep_cost(g);
  return t.c_level_ns + t.c_edge_ns * (double)ef + t.c_pop_ns * (double)nf;
}

// SURVEY 8(d) sweep model, 12 m + 36 n + 4, with n = the rows the sweep carries: rows without in-edges receive
// nothing and are not touched by the single-query sweep (the power method counts the same rows)
uint64_t dense_level_bytes(const pprhip_graph* g) { return 12ull * g->gr->m + 36ull * g->gr->n_nz + 4ull; }

// Compulsory bytes of one sweep: what it has to move when every byte is counted once (pprhip_stats_t.sweep_min_bytes).
// Single query: column indices + row-start bits, every gatherable contribution once (8 B per node with out-edges),
// per row with in-edges the row sum out and in (16 B), the next contribution (8 B) and the residue read and written
// (16 B).  The reserve is touched by crossing rows only and is left out: a lower bound.
uint64_t dense_level_min_bytes(const pprhip_graph* g) {
  const GraphData* D = g->gr;
  return 4ull * D->m + D->m / 8 + 8ull * D->n_src_live + 40ull * D->n_nz;
}
// Batched: the index stream once, every gatherable line c8[v][0..15] once (128 B), per carried row the 128-byte row-sum
// line out and in and the next-contribution line out, and per busy query the residue of every row with in-edges.
uint64_t batch_sweep_min_bytes(const pprhip_graph* P, bool backward, int n_active) {
  const GraphData* D = P->gr;
  const uint64_t rows_nz = backward ? D->n_nz_o : D->n_nz, rows_all = rows_nz + (backward ? D->n_z_o : D->n_zin);
  const uint64_t gather = backward ? (uint64_t)D->n_nz : (uint64_t)D->n_src_live;
  return 4ull * D->m + D->m / 8 + 128ull * gather + 256ull * rows_nz + 128ull * rows_all +
         16ull * rows_nz * (uint64_t)n_active;
}

// smallest frontier (nodes + edges) that runs as Gauss-Seidel sweeps; ~0 when they are switched off
unsigned long long gs_thresh_of(const pprhip_graph* g) {
  if (g->tun.gs_blocks <= 1 || !g->gr->relabeled) return ~0ull;
  return (unsigned long long)std::ceil(g->tun.gs_frac * (double)g->gr->m);
}

// Blocks of the forward sweep (rows = nodes with in-edges in internal order): block b holds the row ordinals
// [jb[b], jb[b + 1]), jb[b] = first ordinal whose in-edge prefix reaches b * m / B, rounded down to a multiple of
// 256 (whole apply tiles), and the in-edges of those rows.  The test twin builds the same blocks
// (oracle/ppr_oracle.c: build_blocks).
const GsBlock* gs_blocks_of(pprhip_graph* g, int* n_blocks) {
  GraphData* D = g->gr;
  const int B = g->tun.gs_blocks;
  *n_blocks = 1;
  if (B <= 1 || !D->relabeled || D->n_nz == 0) return nullptr;
  if (D->gs_plan_B != B) {
    const std::vector<uint32_t>& irp = D->h_in_rp;
    const std::vector<int32_t>& rows = D->h_nz_rows;
    const uint32_t n_nz = D->n_nz;
    std::vector<uint32_t> jb((size_t)B + 1, 0);
    for (int b = 1; b < B; ++b) {
      const uint64_t target = (uint64_t)b * D->m / (uint64_t)B;
      uint32_t lo = 0, hi = n_nz;  // first ordinal whose in-edge prefix (= row start) reaches the target
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)irp[rows[mid]] >= target) hi = mid; else lo = mid + 1;
      }
      const uint32_t j = lo & ~255u;
      jb[b] = std::max(jb[b - 1], j);
    }
    jb[B] = n_nz;
    D->gs_plan.assign((size_t)B, GsBlock{0, 0, 0, 0});
    for (int b = 0; b < B; ++b) {
      GsBlock& K = D->gs_plan[b];
      K.j_lo = jb[b];
      K.j_hi = jb[b + 1];
      K.e_lo = K.j_lo < n_nz ? irp[rows[K.j_lo]] : D->m;
      K.e_hi = K.j_hi < n_nz ? irp[rows[K.j_hi]] : D->m;
    }
    D->gs_plan_B = B;
  }
  *n_blocks = B;
  return D->gs_plan.data();
}

// Windows of the sliced layout (engine.hpp: SlicedLayout) for a sweep cut into the row blocks `blocks` (nullptr: one
// block, every row): per block, for every slice, the edges of the block's rows in that slice; neighbouring ranges are
// joined.  Cached per block count (the blocks of a count are always the same, gs_blocks_of).
static std::mutex g_sl_plan_mu;
const EdgeWindows* sliced_windows_of(pprhip_graph* g, const GsBlock* blocks, int nb) {
  GraphData* D = g->gr;
  SlicedLayout* L = D->sl;
  std::lock_guard<std::mutex> lock(g_sl_plan_mu);
  if (L->plan_B == nb) return L->plan.data();
  const GsBlock whole{0u, D->n_nz, 0ull, (unsigned long long)D->m};
  if (!blocks || nb <= 1) {
    blocks = &whole;
    nb = 1;
  }
  L->plan.assign((size_t)nb, EdgeWindows{});
  for (int b = 0; b < nb; ++b) {
    EdgeWindows& W = L->plan[b];
    W.n = 0;
    for (int sl = 0; sl < L->S; ++sl) {
      const uint32_t* lo = L->h_seg_row.data() + L->seg_base[sl];
      const uint32_t* hi = L->h_seg_row.data() + L->seg_base[sl + 1];
      const size_t g_lo = (size_t)(std::lower_bound(lo, hi, blocks[b].j_lo) - L->h_seg_row.data());
      const size_t g_hi = (size_t)(std::lower_bound(lo, hi, blocks[b].j_hi) - L->h_seg_row.data());
      const unsigned long long e_lo = g_lo < L->seg_base[sl + 1] ? L->h_seg_off[g_lo] : L->edge_base[sl + 1];
      const unsigned long long e_hi = g_hi < L->seg_base[sl + 1] ? L->h_seg_off[g_hi] : L->edge_base[sl + 1];
      if (e_hi <= e_lo) continue;
      if (W.n && W.e_hi[W.n - 1] == e_lo) {
        W.e_hi[W.n - 1] = e_hi;
      } else {
        W.e_lo[W.n] = e_lo;
        W.e_hi[W.n] = e_hi;
        W.n++;
      }
    }
    W.c_pre[0] = 0;
    for (uint32_t w = 0; w < W.n; ++w) {
      W.c_lo[w] = (uint32_t)(W.e_lo[w] / kChunkPad);
      const uint32_t c_hi = (uint32_t)((W.e_hi[w] + kChunkPad - 1) / kChunkPad);
      W.c_pre[w + 1] = W.c_pre[w] + (c_hi - W.c_lo[w]);
    }
  }
  L->plan_B = nb;
  return L->plan.data();
}

// bookkeeping after a dense level: the frontier it produced becomes the current one
void finish_dense(LevelCtx& L, pprhip_stats_t& st, uint64_t level_bytes, uint64_t min_bytes, uint32_t nf_next,
                  uint64_t ef_next) {
  st.sweep_min_bytes += min_bytes;
  // after an entry / in-place sweep the new contributions have reached the later blocks only (nothing is pending
  // when the sweep prepared no node)
  L.gs_dirty = (L.gs_state == kGsEntry || L.gs_state == kGsInPlace) && nf_next > 0;
  L.dense_run++;
  L.ccur ^= 1;
  L.dslot ^= 1;
  L.pslot ^= 1;
  st.dense_levels++;
  st.dense_nodes += L.nf;
  st.dense_edges += L.ef;
  st.push_bytes += level_bytes;
  L.nf = nf_next;
  L.ef = ef_next;
  st.levels++;
  st.enqueues += L.nf;
  st.push_bytes += 5ull * L.nf;
}

// One single-query dense level on the handle's stream, bracketed as PPRHIP_KERNEL_DENSE_PULL.  The sweep writes
// contributions of non-empty rows only.  Rows without in-edges can hold one solely from a phase's seeding, so the
// other buffer is cleared when a dense phase starts and the seeded buffer right after its first level has consumed it.
int launch_dense_pull(pprhip_graph* g, const PushArgs& a, int cc, int out, int ds, bool first_of_phase,
                      const DenseLaunch& dl) {
  if (first_of_phase) PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[cc ^ 1], 0, sizeof(double) * g->gr->n, g->stream));
  ktimer().begin(PPRHIP_KERNEL_DENSE_PULL, dense_level_bytes(g));
  PPRHIP_TRY(launch_dense_level(g, a, cc, out, ds, dl));
  ktimer().end();
  if (first_of_phase) PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[cc], 0, sizeof(double) * g->gr->n, g->stream));
  return PPRHIP_OK;
}

namespace {
// what run_levels works out once per call and both kinds of batch read
struct LevelPlan {
  bool bwd, slot;
  // smallest integer x with (double)x >= dense_frac * m: the device-side form of level_cost()'s test
  unsigned long long dense_thresh;
  unsigned long long gs_thresh;
  const GsBlock* gs_blocks;
  int n_gs;
};
}  // namespace

// A batch of dense levels (cost: the model's cost of the first).  Prepares the level unless a seeding or the batch
// before has; with yield_dense it returns kYield there instead of running it, and kYieldColumn when a pooled workspace
// finds no free column of c8.
static int run_dense_batch(pprhip_graph* g, const PushArgs& a, LevelCtx& L, pprhip_stats_t& st, double* model_cost,
                           bool yield_dense, RoundCut* cut, const LevelPlan& P, double cost) {
  if (!L.dense_prepared && P.slot && g->pooled && !g->has_col) {
    // workspace pool: the level needs a column of c8 (nothing has been decided or queued yet: the driver calls
    // again when one is free)
    int c = 0;
    while (c < kBatch && g->parent->batch->col_owner[c] >= 0) ++c;
    if (c == kBatch) return kYieldColumn;
    g->parent->batch->col_owner[c] = g->ws_index;
    g->slot_index = c;
    g->has_col = true;
  }
  if (model_cost) *model_cost += cost;
  if (cut) cut->had_dense = true;
  if (P.bwd && !P.slot) PPRHIP_TRY(ensure_bwd_layout(g));  // sweep layout over the out-CSR, built on first use
  if (!P.bwd && !P.slot) PPRHIP_TRY(ensure_panel_part(g));  // (graphs with the row-panel copy)
  if (!L.dense_prepared) {
    C8Scope c8(g, false);
    PPRHIP_TRY(c8.rc);
    if (P.slot) {
      if (g->sync) g->sync->c8_enter(g->slot_index);
      L.ccur = g->parent->batch->c8cur;  // the slot's column of the shared array is all-zero here
    } else
      PPRHIP_CHECK_HIP(hipMemsetAsync(g->cdense[L.ccur], 0, sizeof(double) * g->gr->n, g->stream));
    PPRHIP_TRY(launch_sparse_prepare(g, a, L.fcur, 0, L.nf, P.dense_thresh, true, L.ccur, L.dslot,
                                     ((unsigned long long)L.nf << kPackShift) | L.ef));
    PPRHIP_TRY(c8.leave());
    L.dense_prepared = true;
    L.dense_run = 0;
    L.gs_dirty = false;
  }
  // state of this sweep (engine.hpp: GsState; the twin takes the same decision)
  {
    const bool big = (unsigned long long)L.nf + L.ef >= P.gs_thresh;
    L.gs_state = L.gs_dirty ? (big ? kGsInPlace : kGsFlush) : (big ? kGsEntry : kGsJacobi);
  }
  if (yield_dense) return kYield;
  // Dense levels are launched kDenseBatch at a time: level j > 0 of a batch reads its state from a device cell
  // that the level before it wrote (gs_next_state of the frontier it left; kGsNone: nothing left to sweep, the
  // level's kernels return at once), so the host reads the batch's counters back in one round trip.
  PPRHIP_CHECK_HIP(hipMemsetAsync(&g->ctr->dhist[0], 0, sizeof(unsigned long long) * 8 + sizeof(int) * 8, g->stream));
  size_t rec0[kDenseBatch];
  ktimer().reserve(kDenseBatch);
  for (int j = 0; j < kDenseBatch; ++j) {
    const int cc = L.ccur ^ (j & 1), ds = L.dslot ^ (j & 1), out = L.pslot ^ 1 ^ (j & 1);
    DenseLaunch dl;
    dl.blocks = P.gs_blocks;
    dl.n_blocks = P.n_gs;
    dl.state_in = j ? &g->ctr->dstate[j] : nullptr;
    dl.state0 = L.gs_state;
    dl.hist_out = &g->ctr->dhist[j + 1];
    dl.state_out = &g->ctr->dstate[j + 1];
    dl.dense_thresh = P.dense_thresh;
    dl.gs_thresh = P.gs_thresh;
    PPRHIP_TRY(launch_dense_pull(g, a, cc, out, ds, j == 0 && L.dense_run == 0, dl));
    rec0[j] = ktimer().recs.size() - 1;  // (the level's bracket: nothing has been recorded since it opened)
  }
  PPRHIP_TRY(fetch_small(g, &g->ctr->dhist[0], &g->h_ctr->dhist[0], sizeof(unsigned long long) * 8 + sizeof(int) * 8));
  int state = L.gs_state;
  for (int j = 0; j < kDenseBatch; ++j) {
    if (j > 0) {
      // level j ran in the state the device derived from level j - 1's counter: the same function here
      const unsigned long long pk = g->h_ctr->dhist[j];
      state = gs_next_state(state, pk >> kPackShift, pk & kPackMask, P.dense_thresh, P.gs_thresh);
      if (state != g->h_ctr->dstate[j]) {
        set_error("dense batch: level %d ran in state %d, the host expects %d", j, g->h_ctr->dstate[j], state);
        return PPRHIP_ERR_STATE;
      }
      if (state == kGsNone) {
        for (int t = j; t < kDenseBatch; ++t)  // gated-off launches are not levels: keep them out of the class stats
          if (rec0[t] < ktimer().recs.size()) ktimer().recs[rec0[t]].cls = PPRHIP_KERNEL_NONE;
        break;
      }
      if (model_cost) *model_cost += dense_sweep_cost(g);  // a dense level costs the same whatever it pushes
      L.gs_state = state;
    }
    const unsigned long long nx = g->h_ctr->dhist[j + 1];
    finish_dense(L, st, dense_level_bytes(g), dense_level_min_bytes(g), (uint32_t)(nx >> kPackShift), nx & kPackMask);
  }
  return PPRHIP_OK;
}

// A batch of sparse levels (cost: the model's cost of the first).  The first level's frontier travels as a kernel
// argument and its prepare kernel clears the counters of the levels behind it; only after a compaction (which counts
// on the device) the counters are cleared by a fill and read from memory.  Returns kYieldDefer when the caller asked
// for the compaction alone (LevelCtx::defer_compact).
static int run_sparse_batch(pprhip_graph* g, const PushArgs& a, LevelCtx& L, pprhip_stats_t& st, double* model_cost,
                            RoundCut* cut, const LevelPlan& P, double cost) {
  const bool first_prepared = L.dense_prepared || L.compacted;
  unsigned long long pk0 = ((unsigned long long)L.nf << kPackShift) | L.ef;
  if (L.dense_prepared) {
    {
      // A slot beside the sweeps queues this on the compute stream and learns of its end through its mailbox: an
      // event recorded there for the slot's stream to wait on held the compute stream up for ~90 us per compaction
      // (kernel trace: nothing ran between the compaction and the kernel queued right behind the record).
      C8Scope c8(g, false);
      PPRHIP_TRY(c8.rc);
      PPRHIP_CHECK_HIP(hipMemsetAsync(&g->ctr->hist[0], 0, sizeof(unsigned long long) * (kMaxBatch + 1), g->stream));
      // dense-prepared state -> list form; the compaction recounts (dead-end nodes carry no edges)
      PPRHIP_TRY(launch_compact_prepared(g, L.ccur, L.fcur, &g->ctr->hist[0], P.bwd));
      L.compact_seq = 0;
      if (c8.on) PPRHIP_TRY(fetch_begin(g, &g->ctr->hist[0], sizeof(unsigned long long), &L.compact_seq));
      if (c8.on && !L.compact_seq) c8.back = true;  // (no mailbox: the slot's stream waits for an event after all)
      PPRHIP_TRY(c8.leave());
    }
    L.dense_prepared = false;
    L.compacted = true;
    // the column must be read (and handed back zeroed) before another sweep may run
    if (g->sync) PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    if (L.defer_compact) return kYieldDefer;  // (queued ahead of the next sweep; the levels follow beside it)
  }
  if (first_prepared) pk0 = ~0ull;
  if (L.compacted && L.compact_seq) {  // the list must be there before the slot's own stream reads it
    unsigned long long pk = 0;
    PPRHIP_TRY(fetch_end(g, L.compact_seq, &g->ctr->hist[0], &pk, sizeof pk));
    L.compact_seq = 0;
  }
  L.compacted = false;
  if (g->sync) g->sync->release(g->slot_index);
  // the round-cut check looks at the state after exactly one sparse level
  const bool cut_check = cut && cut->enabled && cut->had_dense && !cut->checked;
  const int n_batch = cut_check ? 1 : kMaxBatch;
  // The batch's levels from wg_from on run in ONE launch on one workgroup as long as they stay small
  // (k_sparse_levels_wg): from the first level when that is small itself, else behind one or two levels of the
  // usual two launches each - a frontier of 2^16 entries + edges or more rarely falls below the cap in one level.
  static const bool wg_on = !(hook_env("PPRHIP_SPARSE_WG") && hook_env("PPRHIP_SPARSE_WG")[0] == '0');
  constexpr unsigned long long kWgCap = 4096;
  const unsigned long long size0 = (unsigned long long)L.nf + L.ef;
  // (a seed set lands each level's dead-end mass in a launch of its own between the level's two kernels: no
  // one-workgroup levels)
  const bool seeded = g->seed_on && !P.bwd;
  const int wg_from = (!wg_on || cut_check || seeded) ? n_batch
                      : (!first_prepared && size0 < kWgCap) ? 0
                      : size0 < 65536                        ? 1
                                                             : 2;
  ktimer().begin(PPRHIP_KERNEL_SPARSE_PUSH, 0);
  for (int i = 0; i < std::min(n_batch, wg_from); ++i) {
    const int fb = L.fcur ^ (i & 1);
    poll_idle(g);
    if (!(i == 0 && first_prepared))
      PPRHIP_TRY(launch_sparse_prepare(g, a, fb, i, i == 0 ? L.nf : 32768, P.dense_thresh, false, 0, L.dslot,
                                       i == 0 ? pk0 : ~0ull));
    if (seeded) PPRHIP_TRY(launch_seed_land_sparse(g, a, fb, i, P.dense_thresh, L.dslot, i == 0 ? pk0 : ~0ull));
    PPRHIP_TRY(launch_sparse_push(g, a, fb, i, i == 0 ? L.ef : (1u << 20), P.dense_thresh, L.dslot, i == 0 ? pk0 : ~0ull));
  }
  if (wg_from < n_batch)
    PPRHIP_TRY(launch_sparse_levels_wg(g, a, L.fcur, wg_from, n_batch - 1, P.dense_thresh, kWgCap, L.dslot,
                                       wg_from == 0 ? pk0 : ~0ull));
  ktimer().end();
  PPRHIP_TRY(fetch_small(g, &g->ctr->hist[0], &g->h_ctr->hist[0], sizeof(unsigned long long) * (kMaxBatch + 1)));
  uint64_t batch_bytes = 0;
  int ran = 0;
  for (int i = 0; i < n_batch; ++i) {
    // level i ran with the frontier the host knows (i == 0) or the one level i-1 produced
    const uint32_t nf_i = i == 0 ? L.nf : (uint32_t)(g->h_ctr->hist[i] >> kPackShift);
    const uint64_t ef_i = i == 0 ? L.ef : (g->h_ctr->hist[i] & kPackMask);
    if (i > 0) {
      bool d2 = false;
      const double ci = level_cost(g, nf_i, ef_i, &d2);
      if (nf_i == 0 || d2) break;  // the device stopped here too (level_runs)
      if (i >= wg_from && (unsigned long long)nf_i + ef_i >= kWgCap) break;  // ... too large for the one workgroup
      if (model_cost) *model_cost += ci;
    } else if (model_cost) {
      *model_cost += cost;
    }
    const uint32_t nf_next = (uint32_t)(g->h_ctr->hist[i + 1] >> kPackShift);
    static const bool level_trace = hook_env("PPRHIP_LEVEL_TRACE") != nullptr;  // developer switch: a line per sparse level
    if (level_trace) fprintf(stderr, "[level] mode %d batch-level %d nf %u ef %llu\n", a.mode, i, nf_i, (unsigned long long)ef_i);
    st.pops += nf_i;
    st.edge_pushes += ef_i;
    st.levels++;
    st.enqueues += nf_next;
    batch_bytes += 44ull * nf_i + 28ull * ef_i + 5ull * nf_next;
    ran++;
  }
  st.push_bytes += batch_bytes;
  if (!ktimer().recs.empty() && ktimer().recs.back().cls == PPRHIP_KERNEL_SPARSE_PUSH)
    ktimer().recs.back().bytes = batch_bytes;
  L.nf = (uint32_t)(g->h_ctr->hist[ran] >> kPackShift);
  L.ef = g->h_ctr->hist[ran] & kPackMask;
  if (ran & 1) L.fcur ^= 1;
  if (cut_check) {
    cut->checked = true;
    bool more = true;
    if (!cut->fixed) {
      double sum = 0.0;
      PPRHIP_TRY(device_sum(g, g->residue, &sum));
      cut->rsum = sum * (1 - cut->alpha);
      more = model_cost && *model_cost < cut->c_walk * cut->rsum * cut->omega;
    }
    if (more) {
      cut->taken = true;
      L.nf = 0;  // the rest of this round's frontier waits for the next threshold
      L.ef = 0;
    }
  }
  return PPRHIP_OK;
}

// Runs levels until the frontier is empty.  Dense levels cost one host round trip each; sparse
// levels are launched kMaxBatch at a time and continue on the device (kernels_push.hip).  With
// yield_dense the function prepares a dense level and returns kYield instead of running it: the
// batch driver runs one sweep for every slot waiting at that point and calls back in.
int run_levels(pprhip_graph* g, const PushArgs& a, LevelCtx& L, pprhip_stats_t& st, double* model_cost,
               bool yield_dense, RoundCut* cut) {
  LevelPlan P;
  P.bwd = a.mode == kBackward;
  P.slot = g->parent != nullptr;
  P.dense_thresh = (unsigned long long)std::ceil(g->tun.dense_frac * (double)g->gr->m);
  P.gs_thresh = P.bwd ? ~0ull : gs_thresh_of(g);
  P.n_gs = 1;
  P.gs_blocks = P.gs_thresh != ~0ull ? gs_blocks_of(g, &P.n_gs) : nullptr;
  while (L.nf > 0) {
    bool dense = false;
    double c = level_cost(g, L.nf, L.ef, &dense);
    if (L.gs_dirty && !dense) {  // the contribution array has to be flushed by one more sweep
      dense = true;
      c = dense_sweep_cost(g);
    }
    PPRHIP_TRY(dense ? run_dense_batch(g, a, L, st, model_cost, yield_dense, cut, P, c)
                     : run_sparse_batch(g, a, L, st, model_cost, cut, P, c));
  }
  return PPRHIP_OK;
}

int seed_single(pprhip_graph* g, LevelCtx& L, int32_t node, uint32_t degree) {
  // frontier = {node}; the first node is pushed unconditionally (Forward_Push.java:81-86)
  PPRHIP_TRY(launch_seed_one(g, L.fcur, node));  // (one launch; a 4-byte copy command and a 4-byte fill before)
  L.nf = 1;
  L.ef = degree;
  L.dense_prepared = false;
  L.gs_dirty = false;
  return PPRHIP_OK;
}

// frontier from a predicate over all nodes (round starts)
int seed_scan(pprhip_graph* g, const PushArgs& a, int seed_kind, LevelCtx& L) {
  if (seed_kind == 1) {
    // top-k round starts: one pass that lists the start set, writes the armed bits and lets the parked nodes go, and
    // one read-back of its counter (a start set large enough for a sweep is prepared from the list by run_levels)
    {
      SetupScope setup(g);
      PPRHIP_TRY(launch_seed_list(g, a, 1, L.fcur, &g->ctr->hist[kMaxBatch + 2], true));
    }
    unsigned long long pk = 0;
    PPRHIP_TRY(fetch_small(g, &g->ctr->hist[kMaxBatch + 2], &pk, sizeof pk));
    L.nf = (uint32_t)(pk >> kPackShift);
    L.ef = pk & kPackMask;
    L.dense_prepared = false;
    L.gs_dirty = false;
    return PPRHIP_OK;
  }
  {
    SetupScope setup(g);
    PPRHIP_TRY(launch_count_active(g, a, seed_kind, L.pslot));
  }
  PPRHIP_TRY(read_packed(g, L.pslot, &L.nf, &L.ef));
  L.dense_prepared = false;
  L.gs_dirty = false;
  bool dense = false;
  if (L.nf) (void)level_cost(g, L.nf, L.ef, &dense);
  // (a pooled workspace that holds no column lists the start set instead; run_levels prepares the level from the
  // list once it has one)
  if (dense && g->parent && g->pooled && !g->has_col) dense = false;
  if (dense) {
    C8Scope c8(g, false);
    PPRHIP_TRY(c8.rc);
    if (g->parent) {
      if (g->sync) g->sync->c8_enter(g->slot_index);
      L.ccur = g->parent->batch->c8cur;
    }
    {
      SetupScope setup(g);
      PPRHIP_TRY(launch_seed_dense(g, a, seed_kind, L.ccur, L.pslot, L.dslot));
    }
    PPRHIP_TRY(c8.leave());
    L.dense_prepared = true;
    L.dense_run = 0;
  } else if (L.nf || seed_kind == 1) {
    // seed kind 1 also runs for an empty start set: parked nodes below min_rmax still leave the set
    // (Forward_Push.java:241-247)
    // (its list counter, hist[kMaxBatch + 2], was cleared by the counting pass above)
    {
      SetupScope setup(g);
      PPRHIP_TRY(launch_seed_list(g, a, seed_kind, L.fcur, &g->ctr->hist[kMaxBatch + 2]));
    }
  }
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip
