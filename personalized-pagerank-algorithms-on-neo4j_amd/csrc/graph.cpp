// graph.cpp — a handle's lifecycle: the one-time device bring-up, device and pinned allocations, the lifted graph's
// uploads (pprhip_graph_create; the host half of the lift is lift.cpp) and the layouts made on first use, the
// per-query workspace and its reset, the batch slots and their shared arrays, and the release / destroy / info /
// tuning / result read-out entry points.  The level loop that runs on these is levels.cpp, the single-query entry
// points engine.cpp (shared declarations: engine_internal.hpp).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace pprhip {
namespace detail {

// Kernel arguments in device memory (the HIP runtime's HIP_FORCE_DEV_KERNARG switch, read when the runtime
// initialises): a launch then costs the command processor a read of HBM instead of a read of host memory over PCIe.
// The paths that are chains of short kernels gain 4-10 % (R-MAT 22: top-k one at a time 804 -> 880 queries/s, 16 in
// flight 1 602 -> 1 692, one whole-graph query at a time 94.8 -> 98.5, headline 320 -> 323).  The library does NOT set
// it (rounds 4's load-time setenv is gone: setenv inside a JVM that already runs threads races with their getenv, and
// a library should not change the runtime for the process's other HIP users); the launchers do, before any thread or
// HIP call exists: host/ppr_main.cpp, bench.py, tests/conftest.py, and the java launcher line of INTEGRATION.md.

// One-time work per device: code objects loaded and kernel attributes set by the thread that lifts the
// first graph onto the device, under a lock, so that the launch paths (which worker threads run
// concurrently) never touch function attributes or trigger a first-use module load.
static std::mutex g_dev_init_mu;
static std::vector<char> g_dev_inited;
int init_device_once(int device) {
  std::lock_guard<std::mutex> lk(g_dev_init_mu);
  if ((size_t)device < g_dev_inited.size() && g_dev_inited[device]) return PPRHIP_OK;
  PPRHIP_TRY(init_kernels_push());
  PPRHIP_TRY(init_kernels_dense());
  PPRHIP_TRY(init_kernels_dense_batch());
  PPRHIP_TRY(init_kernels_frontier());
  PPRHIP_TRY(init_kernels_walk());
  PPRHIP_TRY(init_kernels_select());
  PPRHIP_TRY(init_kernels_apbs());
  PPRHIP_TRY(init_kernels_sort());
  PPRHIP_TRY(init_kernels_sweep());
  PPRHIP_TRY(init_kernels_compact());
  PPRHIP_TRY(init_kernels_host());
  PPRHIP_TRY(init_kernels_target());
  PPRHIP_TRY(init_kernels_weighted());
  PPRHIP_TRY(init_kernels_weighted_bwd());
  PPRHIP_TRY(init_kernels_weighted_query());
  PPRHIP_TRY(init_kernels_weighted_batch());
  PPRHIP_TRY(init_kernels_weighted_topk_batch());
  PPRHIP_TRY(init_kernels_weighted_bwd_batch());
  PPRHIP_TRY(init_kernels_weighted_sweep());
  if ((size_t)device >= g_dev_inited.size()) g_dev_inited.resize((size_t)device + 1, 0);
  g_dev_inited[device] = 1;
  return PPRHIP_OK;
}

int alloc_dev(void** p, size_t bytes) {
  // test switch: PPRHIP_FAIL_ALLOC_AFTER=<n> makes the n-th device allocation made while it is set fail as the device
  // running out of memory would (the count starts over whenever the variable is not there)
  static std::atomic<long> armed_count{0};
  if (const char* fe = hook_env("PPRHIP_FAIL_ALLOC_AFTER")) {
    if (armed_count.fetch_add(1) + 1 == atol(fe)) {
      *p = nullptr;
      set_error("hipMalloc(%zu bytes) failed: injected (PPRHIP_FAIL_ALLOC_AFTER)", bytes);
      return PPRHIP_ERR_OOM;
    }
  } else {
    armed_count.store(0);
  }
  hipError_t e = hipMalloc(p, bytes ? bytes : 8);
  if (e != hipSuccess) {
    set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? PPRHIP_ERR_OOM : PPRHIP_ERR_HIP;
  }
  return PPRHIP_OK;
}

// pinned host memory, zeroed (flags: hipHostMallocDefault, or hipHostMallocMapped for memory a kernel writes); not
// counted by PPRHIP_FAIL_ALLOC_AFTER, which addresses device allocations by ordinal
int alloc_pinned(void** p, size_t bytes, unsigned flags) {
  if (hipHostMalloc(p, bytes, flags) != hipSuccess) {
    *p = nullptr;
    set_error(flags & hipHostMallocMapped ? "hipHostMalloc (mapped) failed" : "hipHostMalloc failed");
    return PPRHIP_ERR_OOM;
  }
  std::memset(*p, 0, bytes);
  return PPRHIP_OK;
}

// a host array copied to a device allocation of its own
static int upload(void** dst, const void* src, size_t bytes) {
  PPRHIP_TRY(alloc_dev(dst, bytes));
  if (bytes) PPRHIP_CHECK_HIP(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return PPRHIP_OK;
}

// Uploads the sliced copy of the (internal-order) in-CSR the host half of the lift built (lift.cpp); no layout when
// the source ids fit one slice.
static int upload_sliced_layout(GraphData* D, HostLift& H) {
  if (H.S < 2) return PPRHIP_OK;
  std::unique_ptr<SlicedLayout> L(new (std::nothrow) SlicedLayout());
  if (!L) return PPRHIP_ERR_OOM;
  L->S = H.S;
  L->width = H.width;
  L->n_seg = H.n_seg;
  L->edge_base = std::move(H.edge_base);
  L->seg_base = std::move(H.seg_base);
  L->h_seg_row = std::move(H.seg_row);
  L->h_seg_off = std::move(H.seg_off);
  D->sl = L.release();  // from here on free_graph_data frees what has been allocated
  PPRHIP_TRY(upload((void**)&D->sl->ci, H.sl_ci.data(), sizeof(int32_t) * H.sl_ci.size()));
  PPRHIP_TRY(upload((void**)&D->sl->flags, H.sl_flags.data(), H.sl_flags.size()));
  PPRHIP_TRY(upload((void**)&D->sl->chunk_starts, H.sl_chunk_starts.data(), sizeof(uint32_t) * H.sl_chunk_starts.size()));
  PPRHIP_TRY(upload((void**)&D->sl->seg_row, D->sl->h_seg_row.data(), sizeof(uint32_t) * D->sl->h_seg_row.size()));
  return PPRHIP_OK;
}

static int upload_panel_layout(GraphData* D, HostLift& H) {
  if (!H.pn.n_items) return PPRHIP_OK;
  std::unique_ptr<PanelLayout> L(new (std::nothrow) PanelLayout());
  if (!L) return PPRHIP_ERR_OOM;
  L->n_panels = H.pn.n_panels;
  L->n_items = H.pn.n_items;
  L->n_part = H.pn.n_part;
  L->h_panel_item0 = std::move(H.pn.panel_item0);
  D->pn = L.release();  // from here on free_graph_data frees what has been allocated
  PPRHIP_TRY(upload((void**)&D->pn->src, H.pn.src.data(), sizeof(int32_t) * H.pn.src.size()));
  PPRHIP_TRY(upload((void**)&D->pn->rloc, H.pn.rloc.data(), sizeof(uint16_t) * H.pn.rloc.size()));
  PPRHIP_TRY(upload((void**)&D->pn->items, H.pn.items.data(), sizeof(PanelItem) * H.pn.items.size()));
  PPRHIP_TRY(upload((void**)&D->pn->panels, H.pn.panels.data(), sizeof(PanelDesc) * H.pn.panels.size()));
  return PPRHIP_OK;
}

// the buffer the items of a panel sweep leave their sums in: per handle, on its first forward dense level (a slot runs
// no single-query dense level and has none)
int ensure_panel_part(pprhip_graph* g) {
  if (g->parent || !g->gr->pn || g->pn_part) return PPRHIP_OK;
  // (pn_part last: its presence means both exist; a failed second allocation leaves neither behind)
  PPRHIP_TRY(alloc_dev((void**)&g->pn_ctr, kPanelQueues * sizeof(uint32_t)));
  PPRHIP_CHECK_HIP(hipMemsetAsync(g->pn_ctr, 0, kPanelQueues * sizeof(uint32_t), g->stream));
  const int rc = alloc_dev((void**)&g->pn_part, sizeof(double) * (size_t)g->gr->pn->n_part);
  if (rc != PPRHIP_OK) {
    (void)hipFree(g->pn_ctr);
    g->pn_ctr = nullptr;
  }
  return rc;
}

int reset_query_state(pprhip_graph* g, bool clear_flags, int32_t node) {
  poll_idle(g);
  // the entries the query before could have written are cleared; the new query's passes cover n_act entries
  const uint32_t n_live = g->gr->n_live;
  g->n_act = (n_live && node >= 0 && (uint32_t)node < n_live) ? n_live : g->gr->n;
  const uint32_t clr = std::max(g->n_act, g->n_dirty ? g->n_dirty : g->gr->n);
  g->n_dirty = g->n_act;
  ClearList cl{};  // one launch for all of them (five fill commands before: the device idled between them)
  auto add = [&](void* p, size_t bytes) {
    cl.p[cl.n] = p;
    cl.bytes[cl.n++] = bytes;
  };
  add(g->residue, sizeof(double) * clr);
  add(g->reserve, sizeof(double) * clr);
  add(g->ctr, sizeof(DevCounters));
  if (clear_flags) add(g->flags, clr);
  // the panel sweep's item queues: a level's closing k_dense_reduce zeroes them, but a query whose level stopped between
  // its edge and reduce launches must not leave them to the next one
  if (g->pn_ctr) add(g->pn_ctr, kPanelQueues * sizeof(uint32_t));
  // the top-k estimate is rewritten over the new query's n_act entries only: what the query before left beyond them goes
  if (clr > g->n_act) add(g->est + g->n_act, sizeof(double) * (clr - g->n_act));
  {
    SetupScope setup(g);
    PPRHIP_TRY(launch_clear(g, cl));
  }
  g->mc_phase = g->mc_last_plan = 0;  // (the plan cells were just cleared)
  g->result_in_est = false;
  return PPRHIP_OK;
}

// per-query workspace of a handle (the graph's own, or a batch slot's)
int alloc_workspace(pprhip_graph* G) {
  const uint32_t n = G->gr->n;
  const size_t nd = sizeof(double) * (size_t)n;
  void** dbl[] = {(void**)&G->residue, (void**)&G->reserve, (void**)&G->est, (void**)&G->cF};
  for (void** p : dbl) PPRHIP_TRY(alloc_dev(p, nd));
  if (!G->parent) {  // single-query dense levels; slots use the parent's interleaved arrays
    PPRHIP_TRY(alloc_dev((void**)&G->cdense[0], nd));
    PPRHIP_TRY(alloc_dev((void**)&G->cdense[1], nd));
    PPRHIP_TRY(alloc_dev((void**)&G->acc_nz, nd));
  }
  for (int i = 0; i < 2; ++i) {
    PPRHIP_TRY(alloc_dev((void**)&G->F[i], sizeof(int32_t) * (size_t)n));
    PPRHIP_TRY(alloc_dev((void**)&G->eoff[i], sizeof(uint32_t) * (size_t)n));
  }
  PPRHIP_TRY(alloc_dev((void**)&G->flags, n));
  PPRHIP_TRY(alloc_dev((void**)&G->armed, sizeof(uint32_t) * ((size_t)n / 32 + 2)));
  PPRHIP_CHECK_HIP(hipMemsetAsync(G->armed, 0, sizeof(uint32_t) * ((size_t)n / 32 + 2), G->stream));
  PPRHIP_TRY(alloc_dev((void**)&G->mc_plan_rec, sizeof(WalkPlanRec) * (size_t)n));
  PPRHIP_TRY(alloc_dev((void**)&G->partial, sizeof(double) * 1024));
  PPRHIP_TRY(alloc_dev((void**)&G->hist, sizeof(uint32_t) * 4096));
  {
    const size_t nblk = std::max<size_t>(1024, ((size_t)n + 1 + 255) / 256) + 72;
    PPRHIP_TRY(alloc_dev((void**)&G->blk_pack, sizeof(unsigned long long) * nblk));
    PPRHIP_TRY(alloc_dev((void**)&G->blk_dead, sizeof(double) * nblk));
    PPRHIP_TRY(alloc_dev((void**)&G->blk_ndead, sizeof(uint32_t) * nblk));
  }
  G->sel_cap = 1u << 18;
  PPRHIP_TRY(alloc_dev((void**)&G->sel_blob, kSelHeader + sizeof(SelRec) * (size_t)G->sel_cap));
  PPRHIP_CHECK_HIP(hipMemsetAsync(G->hist, 0, sizeof(uint32_t) * 4096, G->stream));
  PPRHIP_CHECK_HIP(hipMemsetAsync(G->sel_blob, 0, kSelHeader, G->stream));
  PPRHIP_TRY(alloc_dev((void**)&G->ctr, sizeof(DevCounters)));
  PPRHIP_TRY(alloc_pinned((void**)&G->h_ctr, sizeof(DevCounters), hipHostMallocDefault));
  PPRHIP_TRY(alloc_pinned((void**)&G->mail, sizeof(HostMail), hipHostMallocMapped));
  if (hipHostGetDevicePointer((void**)&G->mail_dev, G->mail, 0) != hipSuccess) {
    set_error("hipHostMalloc (mapped) failed");
    return PPRHIP_ERR_OOM;
  }
  G->mail_seq = 0;
  for (auto& e : G->ev)
    if (hipEventCreate(&e) != hipSuccess) {
      set_error("hipEventCreate failed");
      return PPRHIP_ERR_HIP;
    }
  if (!G->parent) {
    PPRHIP_CHECK_HIP(hipMemsetAsync(G->acc_nz, 0, nd, G->stream));
    PPRHIP_CHECK_HIP(hipMemsetAsync(G->cdense[0], 0, nd, G->stream));
    PPRHIP_CHECK_HIP(hipMemsetAsync(G->cdense[1], 0, nd, G->stream));
  }
  PPRHIP_CHECK_HIP(hipMemsetAsync(G->est, 0, nd, G->stream));
  PPRHIP_CHECK_HIP(hipMemsetAsync(G->flags, 0, n, G->stream));
  return reset_query_state(G, true);
}

void free_workspace(pprhip_graph* g) {
  void* ptrs[] = {g->pn_part, g->pn_ctr, g->acc_nz, g->residue, g->reserve, g->est, g->cdense[0], g->cdense[1], g->cF, g->F[0], g->F[1],
                  g->eoff[0], g->eoff[1], g->flags, g->armed, g->mc_plan_rec, g->partial, g->hist, g->sel_blob,
                  g->ctr, g->blk_pack, g->blk_dead, g->blk_ndead};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (g->h_ctr) (void)hipHostFree(g->h_ctr);
  if (g->mail) (void)hipHostFree(g->mail);
  g->mail = g->mail_dev = nullptr;
  if (g->spec_stream) {
    (void)hipStreamSynchronize(g->spec_stream);
    (void)hipStreamDestroy(g->spec_stream);
  }
  if (g->spec_mail) (void)hipHostFree(g->spec_mail);
  if (g->mc_plan_rec2) (void)hipFree(g->mc_plan_rec2);
  g->mc_plan_rec2 = nullptr;
  for (auto& e : g->spec_ev)
    if (e) (void)hipEventDestroy(e);
  g->spec_timer.destroy();
  g->spec_stream = nullptr;
  g->spec_mail = g->spec_mail_dev = nullptr;
  g->spec_ev[0] = g->spec_ev[1] = nullptr;
  for (auto e : g->ev)
    if (e) (void)hipEventDestroy(e);
}

// one batch workspace: slots[w] works on column w % kBatch of the interleaved arrays
static int make_slot(pprhip_graph* P, int w) {
  pprhip_graph* S = new (std::nothrow) pprhip_graph();
  if (!S) return PPRHIP_ERR_OOM;
  P->batch->slots.push_back(S);
  S->parent = P;
  S->slot_index = w % kBatch;
  S->ws_index = w;
  if (hipStreamCreateWithFlags(&S->own_stream, hipStreamNonBlocking) != hipSuccess) {
    set_error("hipStreamCreate failed");
    return PPRHIP_ERR_HIP;
  }
  S->gr = P->gr;  // (the handle's graph itself: a slot holds no copy of any of it)
  S->stream = P->stream;
  S->tun = P->tun;
  PPRHIP_TRY(alloc_workspace(S));
  return PPRHIP_OK;
}

static void drop_slot(pprhip_graph* S) {
  for (auto& ev : S->walk_ev) {
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr;
  }
  for (auto& ev : S->c8_ev) {
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr;
  }
  if (S->col_ev) (void)hipEventDestroy(S->col_ev);
  S->col_ev = nullptr;
  seed_free(S);  // (a workspace's seed table: made by its first seed-set query)
  free_workspace(S);
  S->ktimer.destroy();
  if (S->own_stream) (void)hipStreamDestroy(S->own_stream);
  delete S;
}

int ensure_workspaces(pprhip_graph* P, int count) {
  std::vector<pprhip_graph*>& slots = P->batch->slots;
  while ((int)slots.size() < count) {
    const size_t before = slots.size();
    const int rc = make_slot(P, (int)before);
    if (rc != PPRHIP_OK) {
      // a workspace that could not be completed (out of memory, mostly) must not stay in the list: the driver falls
      // back to the workspaces there are, and a later call tries again from a clean state
      if (slots.size() > before) {
        drop_slot(slots.back());
        slots.pop_back();
      }
      return rc;
    }
  }
  PPRHIP_CHECK_HIP(hipStreamSynchronize(P->stream));
  return PPRHIP_OK;
}

// The apply kernel's row records of one sweep side (BatchState::apply_meta), built once: with the batch state for the
// forward side, and for the backward side as soon as both the batch state and the layout over the out-CSR exist.
static int ensure_apply_meta(pprhip_graph* P, bool backward) {
  BatchState* B = P->batch;
  const GraphData* D = P->gr;
  if (!B || B->apply_meta[backward] || (backward && !D->start_flags_o)) return PPRHIP_OK;
  const uint32_t n_rows = backward ? D->n_nz_o + D->n_z_o : D->n_nz + D->n_zin;
  PPRHIP_TRY(alloc_dev((void**)&B->apply_meta[backward], sizeof(uint4) * apply_meta_rows(n_rows)));
  PPRHIP_TRY(launch_build_apply_meta(P, backward));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(P->stream));
  return PPRHIP_OK;
}

// Batch slots and the interleaved dense-level arrays, created on the first batched call.
static int build_batch(pprhip_graph* P) {
  BatchState* B = P->batch;
  const size_t n = P->gr->n;
  for (int i = 0; i < 2; ++i) {
    PPRHIP_TRY(alloc_dev((void**)&B->c8[i], sizeof(double) * n * kBatch));
    PPRHIP_CHECK_HIP(hipMemsetAsync(B->c8[i], 0, sizeof(double) * n * kBatch, P->stream));
  }
  PPRHIP_TRY(alloc_dev((void**)&B->acc8, sizeof(double) * (n + 1) * kBatch));
  PPRHIP_CHECK_HIP(hipMemsetAsync(B->acc8, 0, sizeof(double) * (n + 1) * kBatch, P->stream));
  PPRHIP_TRY(alloc_dev((void**)&B->prep_bits, sizeof(unsigned long long) * kBatch * (n / 64 + 2)));
  PPRHIP_CHECK_HIP(hipMemsetAsync(B->prep_bits, 0, sizeof(unsigned long long) * kBatch * (n / 64 + 2), P->stream));
  PPRHIP_TRY(alloc_dev((void**)&B->d_slot_args, slot_args_bytes()));
  PPRHIP_TRY(alloc_pinned((void**)&B->h_slot_args, slot_args_bytes(), hipHostMallocDefault));
  std::memset(B->h_slot_args, 0, slot_args_bytes());
#ifdef PPRHIP_TEST_HOOKS
  PPRHIP_TRY(alloc_dev((void**)&B->apply_res_count, sizeof(unsigned long long) * 3));
  PPRHIP_CHECK_HIP(hipMemsetAsync(B->apply_res_count, 0, sizeof(unsigned long long) * 3, P->stream));
#endif
  PPRHIP_TRY(alloc_dev((void**)&B->sweep_out, sizeof(unsigned long long) * kBatch));
  PPRHIP_TRY(alloc_pinned((void**)&B->h_sweep_out, sizeof(unsigned long long) * kBatch, hipHostMallocDefault));
  PPRHIP_TRY(alloc_dev((void**)&B->blk_pack8, sizeof(unsigned long long) * kBatch * kApplyBlocks8));
  PPRHIP_TRY(alloc_dev((void**)&B->blk_dead8, sizeof(double) * kBatch * kApplyBlocks8));
  PPRHIP_TRY(alloc_dev((void**)&B->blk_ndead8, sizeof(uint32_t) * kBatch * kApplyBlocks8));
  PPRHIP_TRY(ensure_apply_meta(P, false));
  PPRHIP_TRY(ensure_apply_meta(P, true));
  for (int s = 0; s < kBatch; ++s) {
    B->col_owner[s] = -1;
    PPRHIP_TRY(make_slot(P, s));
  }
  PPRHIP_CHECK_HIP(hipStreamSynchronize(P->stream));
  return PPRHIP_OK;
}

int ensure_batch(pprhip_graph* P) {
  if (P->batch) return PPRHIP_OK;
  P->batch = new (std::nothrow) BatchState();
  if (!P->batch) return PPRHIP_ERR_OOM;
  const int rc = build_batch(P);
  if (rc != PPRHIP_OK) free_batch(P);  // e.g. out of memory half-way: leave no partial batch state behind
  return rc;
}

void free_batch(pprhip_graph* P) {
  P->ktimer.destroy();  // (the batched sweeps' timer)
  BatchState* B = P->batch;
  if (!B) return;
  if (B->fetch) {
    B->fetch->destroy();
    delete B->fetch;
  }
  free_walk_share(B);
  if (B->walk_stream) (void)hipStreamDestroy(B->walk_stream);
  if (B->slot_stream) (void)hipStreamDestroy(B->slot_stream);
  for (pprhip_graph* S : B->slots) drop_slot(S);
  void* dev[] = {B->c8[0], B->c8[1], B->acc8, B->prep_bits, B->d_slot_args, B->sweep_out, B->blk_pack8, B->blk_dead8,
                 B->blk_ndead8, B->apply_meta[0], B->apply_meta[1]};
  for (void* p : dev)
    if (p) (void)hipFree(p);
#ifdef PPRHIP_TEST_HOOKS
  if (B->apply_res_count) (void)hipFree(B->apply_res_count);
#endif
  if (B->h_slot_args) (void)hipHostFree(B->h_slot_args);
  if (B->h_sweep_out) (void)hipHostFree(B->h_sweep_out);
  delete B;
  P->batch = nullptr;
}

// sweep layout over the out-CSR for batched backward searches (the forward one is built at graph lift)
int ensure_bwd_layout(pprhip_graph* P) {
  GraphData* D = P->gr;
  if (D->start_flags_o) return ensure_apply_meta(P, true);
  const uint32_t n = D->n;
  const uint64_t m = D->m;
  const std::vector<uint32_t>& rp = D->h_out_rp;
  const size_t n_chunks = ((size_t)m + kChunkPad - 1) / kChunkPad;
  std::vector<uint8_t> flags((n_chunks + 1) * (kChunkPad / 8), 0);
  std::vector<uint32_t> chunk_starts(n_chunks + 1, 0);
  std::vector<int32_t> nz, zr;
  for (uint32_t v = 0; v < n; ++v) {
    if (rp[v + 1] == rp[v]) {
      // a row that never receives; it can still hold a contribution of its own when it is a search's target, which
      // only matters to rows that pull from it - so rows that nobody points to are left out of the sweep altogether
      if (D->h_in_rp[v + 1] > D->h_in_rp[v]) zr.push_back((int32_t)v);
      continue;
    }
    nz.push_back((int32_t)v);
    const uint32_t e = rp[v];
    flags[e >> 3] |= (uint8_t)(1u << (e & 7));
    chunk_starts[(size_t)e / kChunkPad + 1]++;
  }
  for (size_t c = 1; c <= n_chunks; ++c) chunk_starts[c] += chunk_starts[c - 1];
  std::vector<unsigned long long> cross(((size_t)n + 63) / 64 + 1, 0ull);
  for (size_t j = 0; j < nz.size(); ++j) {
    const uint32_t v = (uint32_t)nz[j];
    const uint32_t last = rp[v + 1] - 1;
    if (rp[v] / kChunkPad != last / kChunkPad || (last + 1) % kChunkPad == 0 || (uint64_t)last + 1 == m)
      cross[j >> 6] |= 1ull << (j & 63);
  }
  D->n_nz_o = (uint32_t)nz.size();
  D->n_z_o = (uint32_t)zr.size();
  PPRHIP_TRY(upload((void**)&D->chunk_starts_o, chunk_starts.data(), sizeof(uint32_t) * chunk_starts.size()));
  PPRHIP_TRY(upload((void**)&D->nz_rows_o, nz.data(), sizeof(int32_t) * nz.size()));
  PPRHIP_TRY(upload((void**)&D->z_rows_o, zr.data(), sizeof(int32_t) * zr.size()));
  PPRHIP_TRY(upload((void**)&D->cross_bits_o, cross.data(), sizeof(unsigned long long) * cross.size()));
  PPRHIP_TRY(upload((void**)&D->start_flags_o, flags.data(), flags.size()));
  return ensure_apply_meta(P, true);
}

}  // namespace detail
}  // namespace pprhip

extern "C" {

// ------------------------------------------------------------------ graph lift
int pprhip_graph_create(uint32_t n, uint64_t m, const uint32_t* out_rp, const int32_t* out_ci, const uint32_t* in_rp,
                        const int32_t* in_ci, int device, pprhip_graph_t** graph_out) {
  if (!graph_out || !out_rp || (!out_ci && m) || n == 0 || n >= (1u << 28) || m >= (1ull << 32) - 1024) {
    set_error("pprhip_graph_create: bad arguments (n=%u m=%llu; limits n < 2^28, m < 2^32 - 1024)", n,
              (unsigned long long)m);
    return PPRHIP_ERR_INVALID;
  }
  if (out_rp[0] != 0 || out_rp[n] != m) {
    set_error("pprhip_graph_create: out_row_ptr[0] must be 0 and out_row_ptr[n] must equal m");
    return PPRHIP_ERR_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error("pprhip_graph_create: no HIP device available (the engine has no CPU fallback)");
    return PPRHIP_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) {
    set_error("pprhip_graph_create: device %d outside [0, %d)", device, ndev);
    return PPRHIP_ERR_NO_DEVICE;
  }
  PPRHIP_CHECK_HIP(hipSetDevice(device));
  PPRHIP_TRY(init_device_once(device));
  const bool have_in = in_rp && (in_ci || m == 0);
  if (have_in && (in_rp[0] != 0 || in_rp[n] != m)) {
    set_error("pprhip_graph_create: in_row_ptr[0] must be 0 and in_row_ptr[n] must equal m");
    return PPRHIP_ERR_INVALID;
  }
  // ---- the host half (lift.cpp): validation, internal vertex order, both CSRs in that order, sweep layouts
  const auto t_lift0 = std::chrono::steady_clock::now();
  HostLift H;
  try {
    PPRHIP_TRY(lift_host(n, m, out_rp, out_ci, in_rp, in_ci, 0, H));
  } catch (const std::bad_alloc&) {
    set_error("pprhip_graph_create: out of host memory");
    return PPRHIP_ERR_OOM;
  }
  const auto t_lift1 = std::chrono::steady_clock::now();
  std::unique_ptr<pprhip_graph> g(new (std::nothrow) pprhip_graph());
  if (!g) return PPRHIP_ERR_OOM;
  GraphData* D = g->gr = new (std::nothrow) GraphData();
  if (!D) return PPRHIP_ERR_OOM;
  D->device = device;
  D->n = n;
  D->m = m;
  pprhip_tuning_default(&g->tun);
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      D->n_cus = prop.multiProcessorCount;
  }
  D->relabeled = H.relabeled;
  D->h_new2old = std::move(H.new2old);
  D->h_old2new = std::move(H.old2new);
  D->h_out_rp = std::move(H.out_rp);
  D->h_in_rp = std::move(H.in_rp);
  D->h_nz_rows = std::move(H.nz_rows);
  D->n_chunks = H.n_chunks;
  D->n_nz = (uint32_t)D->h_nz_rows.size();
  D->n_zin = (uint32_t)H.zin_rows.size();
  D->n_live = D->relabeled ? D->n_nz + D->n_zin : 0u;  // (ids are the caller's without the relabeling: no bound)
  D->n_src_live = H.n_src_live;

  pprhip_graph* G = g.get();
  int rc = PPRHIP_OK;
  auto fail = [&](int code) {
    pprhip_graph_destroy(g.release());
    return code;
  };
  if ((rc = upload((void**)&D->out_rp, D->h_out_rp.data(), sizeof(uint32_t) * ((size_t)n + 1)))) return fail(rc);
  if ((rc = upload((void**)&D->out_ci, H.out_ci.data(), sizeof(int32_t) * H.out_ci.size()))) return fail(rc);
  if ((rc = upload((void**)&D->out_ext, H.ext.data(), sizeof(unsigned long long) * (size_t)n))) return fail(rc);
  if ((rc = upload((void**)&D->in_rp, D->h_in_rp.data(), sizeof(uint32_t) * ((size_t)n + 1)))) return fail(rc);
  if ((rc = upload((void**)&D->in_ci, H.in_ci.data(), sizeof(int32_t) * H.in_ci.size()))) return fail(rc);
  if ((rc = upload((void**)&D->new2old, D->h_new2old.data(), sizeof(int32_t) * (size_t)n))) return fail(rc);
  if ((rc = upload((void**)&D->old2new, D->h_old2new.data(), sizeof(int32_t) * (size_t)n))) return fail(rc);
  if ((rc = upload((void**)&D->start_flags, H.flags.data(), H.flags.size()))) return fail(rc);
  if ((rc = upload((void**)&D->chunk_starts, H.chunk_starts.data(), sizeof(uint32_t) * H.chunk_starts.size()))) return fail(rc);
  if ((rc = upload((void**)&D->nz_rows, D->h_nz_rows.data(), sizeof(int32_t) * D->h_nz_rows.size()))) return fail(rc);
  if ((rc = upload_sliced_layout(D, H))) return fail(rc);
  if ((rc = upload_panel_layout(D, H))) return fail(rc);
  if (hipStreamCreateWithFlags(&G->stream, hipStreamNonBlocking) != hipSuccess) {
    set_error("hipStreamCreate failed");
    return fail(PPRHIP_ERR_HIP);
  }
  if ((rc = upload((void**)&D->zin_rows, H.zin_rows.data(), sizeof(int32_t) * H.zin_rows.size()))) return fail(rc);
  if ((rc = upload((void**)&D->cross_bits, H.cross.data(), sizeof(unsigned long long) * H.cross.size()))) return fail(rc);
  if (hook_env("PPRHIP_LIFT_DEBUG")) {
    const auto t_up = std::chrono::steady_clock::now();
    fprintf(stderr, "[pprhip lift] host half %.1f ms, uploads %.1f ms\n",
            std::chrono::duration<double, std::milli>(t_lift1 - t_lift0).count(),
            std::chrono::duration<double, std::milli>(t_up - t_lift1).count());
  }
  if ((rc = alloc_dev((void**)&D->walk_rec, sizeof(uint4) * (size_t)m))) return fail(rc);
  if ((rc = launch_build_walk_rec(G))) return fail(rc);
  if ((rc = alloc_workspace(G))) return fail(rc);
  if (hipStreamSynchronize(G->stream) != hipSuccess) {
    set_error("stream sync after graph upload failed");
    return fail(PPRHIP_ERR_HIP);
  }
  *graph_out = g.release();
  return PPRHIP_OK;
}

// the lifted graph and every layout built from it (pprhip_graph_destroy, after everything that uses it)
static void free_graph_data(GraphData* D) {
  free_walk_index(D->widx);
  free_weights(D);  // (the weighted walk index with them)
  void* ptrs[] = {D->walk_rec, D->out_ext, D->out_rp, D->out_ci, D->in_rp, D->in_ci, D->new2old, D->old2new, D->start_flags,
                  D->chunk_starts, D->nz_rows, D->zin_rows, D->cross_bits, D->start_flags_o, D->chunk_starts_o,
                  D->nz_rows_o, D->z_rows_o, D->cross_bits_o, D->survival};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (D->sl) {
    void* sp[] = {D->sl->ci, D->sl->flags, D->sl->chunk_starts, D->sl->seg_row};
    for (void* p : sp)
      if (p) (void)hipFree(p);
    delete D->sl;
  }
  if (D->pn) {
    void* pp[] = {D->pn->src, D->pn->rloc, D->pn->items, D->pn->panels};
    for (void* p : pp)
      if (p) (void)hipFree(p);
    delete D->pn;
  }
  delete D;
}

static void free_all_pair(pprhip_graph* g) {
  void* ptrs[] = {g->apbs_dense.ws, g->apbs_xl.ws, g->apbs_board, g->in_rec};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  g->apbs_dense = g->apbs_xl = pprhip::ApbsWorkspace{};  // (allpair.cpp sizes and allocates the workspaces it does not find)
  g->apbs_board = g->in_rec = nullptr;
  free_weighted_in_rec(g->gr);
  if (g->ix_stage) (void)hipHostFree(g->ix_stage);
  g->ix_stage = nullptr;
  g->ix_stage_bytes = 0;
}

int pprhip_graph_release(pprhip_graph_t* g, unsigned what) {
  PPRHIP_TRY(check_graph(g, "pprhip_graph_release"));
  if (what & ~(PPRHIP_RELEASE_ALL_PAIR | PPRHIP_RELEASE_BATCH | PPRHIP_RELEASE_WALK_INDEX | PPRHIP_RELEASE_SWEEP |
               PPRHIP_RELEASE_SPARSE | PPRHIP_RELEASE_WEIGHTS | PPRHIP_RELEASE_WEIGHTED_WALK_INDEX)) {
    set_error("pprhip_graph_release: unknown flag in %u", what);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  if (what & PPRHIP_RELEASE_ALL_PAIR) free_all_pair(g);
  if (what & PPRHIP_RELEASE_BATCH) free_batch(g);
  if (what & PPRHIP_RELEASE_WALK_INDEX) PPRHIP_TRY(pprhip_walk_index_drop(g));
  if (what & PPRHIP_RELEASE_SWEEP) free_sweep(g);
  if (what & PPRHIP_RELEASE_SPARSE) free_sparse(g);
  if (what & PPRHIP_RELEASE_WEIGHTED_WALK_INDEX) PPRHIP_TRY(pprhip_weighted_walk_index_drop(g));
  if (what & PPRHIP_RELEASE_WEIGHTS) free_weights(g->gr);
  return PPRHIP_OK;
}

void pprhip_graph_destroy(pprhip_graph_t* g) {
  if (!g) return;
  if (g->stream_obj) stream_detach(g->stream_obj);  // (its driver thread uses the handle; the stream object stays its owner's)
  (void)hipSetDevice(g->gr->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  free_batch(g);
  free_all_pair(g);
  seed_free(g);
  free_sweep(g);
  free_sparse(g);
  free_workspace(g);
  if (g->stream) (void)hipStreamDestroy(g->stream);
  free_graph_data(g->gr);
  delete g;
}

int pprhip_device_memory(const pprhip_graph_t* g, uint64_t* free_bytes, uint64_t* total_bytes) {
  if (!g) {
    set_error("pprhip_device_memory: null handle");
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_CHECK_HIP(hipSetDevice(g->gr->device));
  size_t f = 0, t = 0;
  PPRHIP_CHECK_HIP(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = (uint64_t)f;
  if (total_bytes) *total_bytes = (uint64_t)t;
  return PPRHIP_OK;
}

int pprhip_graph_info(const pprhip_graph_t* g, uint32_t* n, uint64_t* m, int* device) {
  if (!g) {
    set_error("pprhip_graph_info: null graph handle");
    return PPRHIP_ERR_INVALID;
  }
  if (n) *n = g->gr->n;
  if (m) *m = g->gr->m;
  if (device) *device = g->gr->device;
  return PPRHIP_OK;
}

int pprhip_graph_set_tuning(pprhip_graph_t* g, const pprhip_tuning_t* t) {
  if (!g || !t) {
    set_error("pprhip_graph_set_tuning: null argument");
    return PPRHIP_ERR_INVALID;
  }
  pprhip_tuning_t d;
  pprhip_tuning_default(&d);
  g->tun = *t;
  if (!(g->tun.c_walk_ns > 0)) g->tun.c_walk_ns = d.c_walk_ns;
  if (!(g->tun.c_edge_ns > 0)) g->tun.c_edge_ns = d.c_edge_ns;
  if (!(g->tun.c_pop_ns > 0)) g->tun.c_pop_ns = d.c_pop_ns;
  if (!(g->tun.c_level_ns > 0)) g->tun.c_level_ns = d.c_level_ns;
  if (!(g->tun.c_dense_edge_ns > 0)) g->tun.c_dense_edge_ns = d.c_dense_edge_ns;
  if (!(g->tun.c_dense_node_ns > 0)) g->tun.c_dense_node_ns = d.c_dense_node_ns;
  if (!(g->tun.dense_frac > 0)) g->tun.dense_frac = d.dense_frac;
  if (g->tun.max_rounds <= 0) g->tun.max_rounds = d.max_rounds;
  if (g->tun.max_halvings <= 0) g->tun.max_halvings = d.max_halvings;
  if (!(g->tun.halving_ratio > 0)) g->tun.halving_ratio = d.halving_ratio;  // a value <= 1 switches the rule off
  if (g->tun.prior_levels == 0) g->tun.prior_levels = d.prior_levels;        // negative: off
  if (g->tun.gs_blocks <= 0) g->tun.gs_blocks = d.gs_blocks;                  // 1: plain Jacobi sweeps
  if (g->tun.gs_blocks > 64) g->tun.gs_blocks = 64;
  if (!(g->tun.gs_frac > 0)) g->tun.gs_frac = d.gs_frac;
  return PPRHIP_OK;
}

int pprhip_graph_get_tuning(const pprhip_graph_t* g, pprhip_tuning_t* t) {
  if (!g || !t) {
    set_error("pprhip_graph_get_tuning: null argument");
    return PPRHIP_ERR_INVALID;
  }
  *t = g->tun;
  return PPRHIP_OK;
}

int pprhip_get_reserve(pprhip_graph_t* g, double* out) {
  PPRHIP_TRY(check_graph(g, "pprhip_get_reserve"));
  if (!out) {
    set_error("pprhip_get_reserve: null output");
    return PPRHIP_ERR_INVALID;
  }
  return copy_out(g, g->result_in_est ? g->est : g->reserve, out);
}

int pprhip_get_residue(pprhip_graph_t* g, double* out) {
  PPRHIP_TRY(check_graph(g, "pprhip_get_residue"));
  if (!out) {
    set_error("pprhip_get_residue: null output");
    return PPRHIP_ERR_INVALID;
  }
  return copy_out(g, g->residue, out);
}

}  // extern "C"
