// allpair.cpp — All-Pair-Backward-Search (Base_Whole_Graph.preprocessing): the record store the searches' entries are
// collected in on the device, the driver of the search tiers (all_pair_collect; the tiers: kernels_apbs.hip),
// pprhip_all_pair_backward and pprhip_weighted_all_pair_backward.  The index the entries end up in is index.cpp's.
// The weighted call is the same driver with ApbsCall::weighted set: the table and dense tiers read the weighted in-edge
// records, and every search they give up is a whole-vector weighted backward push (the batch slots are unweighted).
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <system_error>
#include <thread>

#include <unistd.h>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace pprhip {
namespace detail {

// ---- the record store: the searches' entries stay in HBM as 16-byte records until the index finalisation (single-GPU
// call) or the exchange by owner of the source (sharded call).  Entries that a tier hands over from host memory have
// the same layout, so they go up in one copy.
static_assert(sizeof(Triple) == sizeof(TripleRec), "host and device entries share one layout");
int TripleStore::reserve(pprhip_graph* g, unsigned long long extra) {
  if (count + extra <= cap) return PPRHIP_OK;
  unsigned long long ncap = std::max<unsigned long long>(cap * 2, std::max<unsigned long long>(count + extra, 1ull << 20));
  TripleRec* nrec = nullptr;
  PPRHIP_TRY(alloc_dev((void**)&nrec, sizeof(TripleRec) * ncap));
  if (count)
    PPRHIP_CHECK_HIP(hipMemcpyAsync(nrec, rec, sizeof(TripleRec) * count, hipMemcpyDeviceToDevice, g->stream));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  if (rec) (void)hipFree(rec);
  rec = nrec;
  cap = ncap;
  return PPRHIP_OK;
}
int TripleStore::take_device(pprhip_graph* g, const TripleRec* d_rec, unsigned long long n_new) {
  PPRHIP_TRY(reserve(g, n_new));
  PPRHIP_CHECK_HIP(hipMemcpyAsync(rec + count, d_rec, sizeof(TripleRec) * n_new, hipMemcpyDeviceToDevice, g->stream));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));  // the source buffer is reused by the next pass
  count += n_new;
  return PPRHIP_OK;
}
int TripleStore::take_host(pprhip_graph* g, std::vector<Triple>& more) {
  if (more.empty()) return PPRHIP_OK;
  PPRHIP_TRY(reserve(g, more.size()));
  PPRHIP_CHECK_HIP(hipMemcpyAsync(rec + count, more.data(), sizeof(TripleRec) * more.size(), hipMemcpyHostToDevice,
                                  g->stream));
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  count += more.size();
  return PPRHIP_OK;
}
TripleStore::~TripleStore() {
  if (rec) (void)hipFree(rec);
}

namespace {

template <class T>
struct FreeOnExit {  // frees a device buffer on every exit, error returns included
  T*& p;
  ~FreeOnExit() {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
};

// ---- one call's state: what every tier's passes share.  The five device buffers live as long as the searches on the
// kernels_apbs.hip tiers do (all_pair_collect frees them before tier 3 takes its own memory).
struct ApbsCall {
  pprhip_graph* g;
  double alpha, threshold;
  uint32_t t_begin, n_targets;
  TripleStore& store;
  pprhip_stats_t& st;
  bool debug;  // developer switch PPRHIP_APBS_DEBUG: phase times and per-workgroup timers on stderr
  bool weighted;  // the searches run over P(u, v) = w / W(u) (GraphData::in_wrec, weighted_backward_search_whole)
  ApbsBuffers B;
  unsigned long long h_cells[kApCells];
  std::vector<int32_t> h_ovf;

  int alloc_buffers() {
    // room for the entries of one pass over the range (16 bytes each; 2 GB at most): a search that finds the buffer
    // full is not run at all but listed for the next pass
    // The buffer must hold what ONE search can emit (up to n entries: a hub's column), or that search would find it
    // full on every pass: until round 5 a range of a few hub targets - 6 of R-MAT 18's in a work-weighted rank's share -
    // was sized for 65 536 entries, the hubs' searches were repeated a thousand times (44 G edge pushes) and then
    // dropped without an error.  Four entries per node also keeps a range of hubs from running pass after pass.
    B.out_cap = std::min<unsigned long long>(
        1ull << 27, std::max<unsigned long long>(std::max<unsigned long long>(1ull << 16, 16ull * n_targets), 4ull * g->gr->n + 1024));
    const size_t list_bytes = sizeof(int32_t) * std::max<uint32_t>(1, n_targets);
    PPRHIP_TRY(alloc_dev((void**)&B.cells, sizeof(unsigned long long) * kApCells));
    PPRHIP_TRY(alloc_dev((void**)&B.out_rec, sizeof(TripleRec) * B.out_cap));
    PPRHIP_TRY(alloc_dev((void**)&B.overflow, list_bytes));
    // (tier 1 over a range: the list of targets with in-edges and the small table's give-ups, kernels_apbs.hip)
    PPRHIP_TRY(alloc_dev((void**)&B.list0, list_bytes));
    PPRHIP_TRY(alloc_dev((void**)&B.list1, list_bytes));
    return PPRHIP_OK;
  }
  void free_buffers() {
    void** p[] = {(void**)&B.cells, (void**)&B.out_rec, (void**)&B.overflow, (void**)&B.list0, (void**)&B.list1};
    for (void** q : p) {
      if (*q) (void)hipFree(*q);
      *q = nullptr;
    }
  }
  ~ApbsCall() { free_buffers(); }
};

// runs one tier over `list` (or the range when list is empty and use_range) until every target
// has either produced its triples or landed in `give_up`
int run_tier(ApbsCall& c, bool dense_tier, std::vector<int32_t> list, bool use_range, std::vector<int32_t>& give_up) {
  pprhip_graph* g = c.g;
  ApbsBuffers& B = c.B;
  pprhip_stats_t& st = c.st;
  const unsigned long long* h_cells = c.h_cells;
  int32_t* d_list = nullptr;
  FreeOnExit<int32_t> list_guard{d_list};
  for (int pass = 0; pass < 1000; ++pass) {
    const uint32_t cnt = use_range ? c.n_targets : (uint32_t)list.size();
    if (cnt == 0) break;
    if (!use_range) {
      if (!d_list) PPRHIP_TRY(alloc_dev((void**)&d_list, sizeof(int32_t) * list.size()));
      PPRHIP_CHECK_HIP(hipMemcpyAsync(d_list, list.data(), sizeof(int32_t) * cnt, hipMemcpyHostToDevice, g->stream));
    }
    unsigned long long init[kApCells] = {};
    init[kApOutValid] = ~0ull;
    PPRHIP_CHECK_HIP(hipMemcpyAsync(B.cells, init, sizeof init, hipMemcpyHostToDevice, g->stream));
    if (dense_tier)  // every board entry closed, nothing posted
      PPRHIP_CHECK_HIP(hipMemsetAsync(B.board, 0, apbs_board_bytes(B.ws_blocks), g->stream));
    ktimer().begin(PPRHIP_KERNEL_BACKWARD_BATCH, 0);
    PPRHIP_TRY(launch_apbs(g, c.weighted, dense_tier, use_range ? nullptr : d_list, c.t_begin, cnt, c.alpha, c.threshold, B));
    ktimer().end();
    PPRHIP_CHECK_HIP(hipMemcpyAsync(c.h_cells, B.cells, sizeof c.h_cells, hipMemcpyDeviceToHost, g->stream));
    PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    if (h_cells[kApAbort]) {
      set_error("All-Pair dense tier: a workgroup waited more than 30 s for the chunks of a posted level (launch aborted)");
      return PPRHIP_ERR_STATE;
    }
    const unsigned long long valid = std::min(std::min(h_cells[kApOutCount], h_cells[kApOutValid]), B.out_cap);
    st.pops += h_cells[kApPops];
    st.edge_pushes += h_cells[kApEdges];
    // (an edge: its record - 8 bytes, 16 with a weight - and the read-modify-write of a residue)
    const uint64_t bytes = 44ull * h_cells[kApPops] + (c.weighted ? 36ull : 28ull) * h_cells[kApEdges] + 16ull * valid;
    st.push_bytes += bytes;
    if (!ktimer().recs.empty()) ktimer().recs.back().bytes = bytes;
    if (valid) PPRHIP_TRY(c.store.take_device(g, B.out_rec, valid));
    std::vector<int32_t> again;
    const unsigned long long novf = h_cells[kApOverflowCount];
    if (novf) {
      c.h_ovf.resize(novf);
      PPRHIP_CHECK_HIP(hipMemcpy(c.h_ovf.data(), B.overflow, sizeof(int32_t) * novf, hipMemcpyDeviceToHost));
      for (int32_t x : c.h_ovf) {
        if (x >= 0) give_up.push_back(x);  // table too small for this target
        else again.push_back(-(x + 1));    // triple buffer was full: same tier again
      }
    }
    // a search that found the buffer full although it came first in an empty one cannot ever fit: an error, not a
    // silent loss of its entries (a pass that emitted nothing and still lists searches for another pass)
    if (!again.empty() && valid == 0 && again.size() == (use_range ? (size_t)c.n_targets : list.size())) {
      set_error("All-Pair: a search yields more than the %llu entries the record buffer holds", B.out_cap);
      return PPRHIP_ERR_STATE;
    }
    list.swap(again);
    use_range = false;
    if (d_list && list.size()) {
      (void)hipFree(d_list);
      d_list = nullptr;
    }
    if (pass == 999 && !list.empty()) {
      set_error("All-Pair: %zu searches still waited for room in the record buffer after 1000 passes", list.size());
      return PPRHIP_ERR_STATE;
    }
  }
  return PPRHIP_OK;
}

// in-edge records for both tiers' edge loops (8 B per edge; stays with the handle)
int ensure_in_rec(pprhip_graph* g) {
  if (g->in_rec) return PPRHIP_OK;
  void* rec = nullptr;
  FreeOnExit<void> rec_guard{rec};
  PPRHIP_TRY(alloc_dev(&rec, sizeof(unsigned long long) * std::max<uint64_t>(1, g->gr->m)));
  PPRHIP_TRY(launch_build_in_rec(g, rec));
  g->in_rec = rec;
  rec = nullptr;
  return PPRHIP_OK;
}

// ... and their weighted twin {source, w / W(source)} (16 B per edge; stays with the lifted graph's weights)
int ensure_weighted_in_rec(pprhip_graph* g) {
  GraphData* D = g->gr;
  if (D->in_wrec) return PPRHIP_OK;
  void* rec = nullptr;
  FreeOnExit<void> rec_guard{rec};
  const uint64_t bytes = 16ull * std::max<uint64_t>(1, D->m);
  PPRHIP_TRY(alloc_dev(&rec, bytes));
  PPRHIP_TRY(launch_build_in_rec_w(g, rec));
  D->in_wrec = rec;
  D->in_wrec_bytes = 16ull * D->m;
  rec = nullptr;
  return PPRHIP_OK;
}

// ---- dense workspaces, one per workgroup in flight (kernels_apbs.hip): 16n bytes of vectors + lists.  The lists hold
// what a search may list before it is handed on: nodes whose residue left zero (clean-up; on overflow the whole vector
// is cleared instead) and a level's frontier.  The workspaces stay with the handle: allocating and zeroing gigabytes
// per call would cost more than the searches of a small target range.
// W as want_first workspaces with lists of cap_t / cap_f, or - a device that cannot spare them all runs the tier with
// fewer workgroups in flight - half as many, down to want_least; W.blocks stays 0 (no error) when even those do not fit.
int ensure_apbs_workspace(pprhip_graph* g, ApbsWorkspace& W, uint32_t want_first, uint32_t want_least, uint32_t cap_t,
                          uint32_t cap_f, const char* what) {
  if (W.blocks) return PPRHIP_OK;
  const size_t per = apbs_dense_bytes(g->gr->n, g->gr->m, cap_t, cap_f, g->apbs_chunk);
  uint32_t want = want_first;
  int rc = PPRHIP_ERR_OOM;
  for (; want >= want_least; want /= 2) {
    rc = alloc_dev((void**)&W.ws, (size_t)want * per);
    if (rc != PPRHIP_ERR_OOM) break;
    (void)hipGetLastError();
  }
  if (rc == PPRHIP_ERR_OOM) return PPRHIP_OK;
  PPRHIP_TRY(rc);
  if (hipMemsetAsync(W.ws, 0, (size_t)want * per, g->stream) != hipSuccess) {
    (void)hipFree(W.ws);
    W.ws = nullptr;
    set_error("All-Pair: clearing the %s workspaces failed", what);
    return PPRHIP_ERR_HIP;
  }
  W.blocks = want;
  W.cap_t = cap_t;
  W.cap_f = cap_f;
  return PPRHIP_OK;
}

// the dense tier's own workspaces and the board its workgroups post levels on, on first use
int ensure_dense_workspaces(pprhip_graph* g) {
  ApbsWorkspace& W = g->apbs_dense;
  if (W.blocks) return PPRHIP_OK;
  // (PPRHIP_APBS_CAP_T / _CAP_F shrink the lists so that tests reach the overflow paths on small graphs,
  // PPRHIP_APBS_CHUNK the chunks of a level's edge space so that small graphs' levels are shared too)
  const char* e_t = hook_env("PPRHIP_APBS_CAP_T");
  const char* e_f = hook_env("PPRHIP_APBS_CAP_F");
  const char* e_c = hook_env("PPRHIP_APBS_CHUNK");
  g->apbs_chunk = e_c ? (uint32_t)std::max(16, atoi(e_c)) : apbs_default_chunk();
  const uint32_t cap_t = e_t ? (uint32_t)std::max(1, atoi(e_t)) : std::min<uint32_t>(g->gr->n, 1u << 20) + 4096u;
  const uint32_t cap_f = e_f ? (uint32_t)std::max(1, atoi(e_f)) : std::min<uint32_t>(g->gr->n, 1u << 20) + 64u;
  const char* per_cu = hook_env("PPRHIP_APBS_WGS_PER_CU");
  const uint32_t want = (uint32_t)g->gr->n_cus * (uint32_t)std::max(1, std::min(2, per_cu ? atoi(per_cu) : 1));
  PPRHIP_TRY(ensure_apbs_workspace(g, W, want, 8, cap_t, cap_f, "dense"));
  if (!W.blocks) return PPRHIP_OK;
  const int rc = alloc_dev(&g->apbs_board, apbs_board_bytes(W.blocks));
  if (rc != PPRHIP_OK) {
    (void)hipFree(W.ws);
    W = ApbsWorkspace{};
  }
  return rc == PPRHIP_ERR_OOM ? PPRHIP_OK : rc;
}

// the next dense passes of this call run on W's workspaces, every workgroup of the dense tier helping with their levels
void use_workspace(ApbsBuffers& B, const pprhip_graph* g, const ApbsWorkspace& W) {
  B.ws = W.ws;
  B.ws_blocks = W.blocks;
  B.cap_t = W.cap_t;
  B.cap_f = W.cap_f;
  B.chunk = g->apbs_chunk;
  B.helpers = g->apbs_dense.blocks;
  B.board = g->apbs_board;
}

// targets with the most in-edges first: the searches that push the most edges start the level-1 fan-out from
// hubs, and a workgroup that draws such a search last would finish long after the others
// (a stable counting sort by in-degree, degrees from 65535 up in one bucket that is sorted on its own: a
// comparison sort of half a million ids with two indirections per comparison was 15-40 ms of every pass)
void order_by_in_degree(const pprhip_graph* g, std::vector<int32_t>& list) {
  const std::vector<uint32_t>& irp = g->gr->h_in_rp;
  const std::vector<int32_t>& o2n = g->gr->h_old2new;
  constexpr uint32_t kCapDeg = 65535;
  const size_t L = list.size();
  std::vector<uint32_t> deg(L);
  std::vector<uint32_t> at((size_t)kCapDeg + 2, 0);
  for (size_t i = 0; i < L; ++i) {
    const int32_t a = g->gr->relabeled ? o2n[list[i]] : list[i];
    deg[i] = irp[a + 1] - irp[a];
    at[kCapDeg - std::min(deg[i], kCapDeg) + 1]++;  // bucket 0: the largest degrees
  }
  for (uint32_t b = 0; b <= kCapDeg; ++b) at[b + 1] += at[b];
  const uint32_t n_top = at[1];
  std::vector<int32_t> sorted(L);
  std::vector<uint32_t> sdeg(n_top);
  for (size_t i = 0; i < L; ++i) {
    const uint32_t b = kCapDeg - std::min(deg[i], kCapDeg);
    const uint32_t pos = at[b]++;
    sorted[pos] = list[i];
    if (b == 0) sdeg[pos] = deg[i];
  }
  if (n_top > 1) {  // the top bucket by exact degree (stable)
    std::vector<uint32_t> idx(n_top);
    for (uint32_t i = 0; i < n_top; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return sdeg[x] > sdeg[y]; });
    std::vector<int32_t> top(n_top);
    for (uint32_t i = 0; i < n_top; ++i) top[i] = sorted[idx[i]];
    std::copy(top.begin(), top.end(), sorted.begin());
  }
  list.swap(sorted);
}

// ---- developer switch PPRHIP_APBS_DEBUG: per-workgroup timers and a progress word in HOST memory (12 words for every
// workgroup of a dense launch, kernels_apbs.hip), there while this object is
struct ApbsDebugRows {
  ApbsBuffers& B;
  const uint32_t rows;
  ApbsDebugRows(ApbsBuffers& B_, bool on) : B(B_), rows(std::max(B_.ws_blocks, B_.helpers)) {
    if (on && hipHostMalloc((void**)&B.dbg, sizeof(unsigned long long) * 12 * rows, hipHostMallocMapped) == hipSuccess)
      std::memset(B.dbg, 0, sizeof(unsigned long long) * 12 * rows);
  }
  ~ApbsDebugRows() {
    if (B.dbg) (void)hipHostFree(B.dbg);
    B.dbg = nullptr;
  }
  // the columns' sums over the workgroups of the last launch; with_ends: also who owned the most edges and how far
  // apart the workgroups ended
  void print(const char* label, bool with_ends) const {
    if (!B.dbg) return;
    const unsigned long long* h = B.dbg;
    unsigned long long tot[8] = {0}, t_end_max = 0, t_end_min = ~0ull, e_max = 0;
    for (uint32_t w = 0; w < rows; ++w) {
      if (!h[12 * w + 8]) continue;  // (took no part)
      for (int i = 0; i < 8; ++i) tot[i] += h[12 * w + i];
      t_end_max = std::max(t_end_max, h[12 * w + 8]);
      t_end_min = std::min(t_end_min, h[12 * w + 8]);
      e_max = std::max(e_max, h[12 * w + 1]);
    }
    fprintf(stderr, "%s searches %llu edges %llu", label, tot[0], tot[1]);
    if (with_ends) fprintf(stderr, " (max owned by one workgroup %llu)", e_max);
    fprintf(stderr, "; workgroup-ms in pops+scans %.1f own chunks %.1f waiting for helpers %.1f emit %.1f clear %.1f helping / idle %.1f",
            tot[2] / 1e5, tot[3] / 1e5, tot[4] / 1e5, tot[5] / 1e5, tot[6] / 1e5, tot[7] / 1e5);
    if (with_ends) fprintf(stderr, "; first workgroup ended %.2f ms before the last", (t_end_max - t_end_min) / 1e5);
    fprintf(stderr, "\n");
  }
};

// ... and a watchdog thread that prints the progress words and ends the process when the tier has not come back
// after 20 s (a kernel that never ends would otherwise only be seen as a process that cannot be killed)
struct ApbsWatchdog {
  std::mutex wd_mu;
  std::condition_variable wd_cv;
  bool wd_done = false;
  std::thread watchdog;
  ApbsWatchdog(const unsigned long long* rows, uint32_t nb) {
    if (rows) watchdog = std::thread(&ApbsWatchdog::watch, this, rows, nb);
  }
  ~ApbsWatchdog() {
    if (!watchdog.joinable()) return;
    {
      std::lock_guard<std::mutex> lk(wd_mu);
      wd_done = true;
    }
    wd_cv.notify_all();
    watchdog.join();
  }
  void watch(const unsigned long long* rows, uint32_t nb) {
    std::unique_lock<std::mutex> lk(wd_mu);
    if (wd_cv.wait_for(lk, std::chrono::seconds(20), [&] { return wd_done; })) return;
    fprintf(stderr, "[apbs dense] no end after 20 s; workgroup: stage/detail (1 target, 2 pops, 3 own chunk, 4 waiting "
                    "for helpers, 5 local chunks, 6 emit, 7 clear, 8 idle, 9 helping owner<<16|chunk, 10 out)\n");
    for (uint32_t w = 0; w < nb; ++w)
      if (rows[12 * w + 9])
        fprintf(stderr, "%u: %llu/%llu%s", w, rows[12 * w + 9] >> 32, rows[12 * w + 9] & 0xffffffffull,
                (w % 8 == 7) ? "\n" : "   ");
    fprintf(stderr, "\n");
    fflush(stderr);
    _exit(3);
  }
};

// ---- the dense tier for a list of targets (workspaces on first use); what outgrows its lists is appended to to_tier3
int dense_tier(ApbsCall& c, std::vector<int32_t>& list, std::vector<int32_t>& to_tier3) {
  pprhip_graph* g = c.g;
  PPRHIP_TRY(ensure_dense_workspaces(g));
  if (!g->apbs_dense.blocks) {  // no memory for the dense tier: everything runs on the batch slots
    to_tier3.insert(to_tier3.end(), list.begin(), list.end());
    return PPRHIP_OK;
  }
  use_workspace(c.B, g, g->apbs_dense);
  order_by_in_degree(g, list);
  ApbsDebugRows dbg(c.B, c.debug);
  int rc;
  {
    ApbsWatchdog wd(c.B.dbg, g->apbs_dense.blocks);
    rc = run_tier(c, true, list, false, to_tier3);
  }
  dbg.print("[apbs dense]", true);
  return rc;
}

// ---- A handful of searches that outgrew the dense tier's lists (R-MAT 22: the one target with 160 K in-edges, whose
// search pushes 300 M edges) run best one at a time on the handle's OWN vectors with the whole chip behind each level:
// levels that touch a large part of the graph as pull sweeps over the out-CSR (no atomics at all), the others as sparse
// pushes - pprhip_backward_push's path.  Measured (tools/exp/apbs_big_searches.py): 2.5 ms of device time for that
// target against 158 ms in the full-size pass below, where one workgroup owns the search and the others help with its
// levels at the rate of memory-side atomics.  The entries go from the reserve vector into records on the device.
// every: whatever their number (the weighted call's last tier: what the dense and full-size passes gave up)
int whole_searches(ApbsCall& c, std::vector<int32_t>& to_tier3, bool every) {
  pprhip_graph* g = c.g;
  pprhip_stats_t& st = c.st;
  const char* whole_env = hook_env("PPRHIP_APBS_WHOLE");
  const size_t whole_max = whole_env ? (size_t)std::max(0, atoi(whole_env)) : 256;
  const bool run = !to_tier3.empty() && (every || to_tier3.size() <= whole_max);
  if (!run) return PPRHIP_OK;
  TripleRec* d_rec = nullptr;
  unsigned long long* d_cnt = nullptr;
  FreeOnExit<TripleRec> rec_guard{d_rec};
  FreeOnExit<unsigned long long> cnt_guard{d_cnt};
  const unsigned long long cap = std::max<uint32_t>(act_n(g), g->gr->n);
  PPRHIP_TRY(alloc_dev((void**)&d_rec, sizeof(TripleRec) * cap));
  PPRHIP_TRY(alloc_dev((void**)&d_cnt, sizeof(unsigned long long)));
  const std::vector<int32_t>& o2n = g->gr->h_old2new;
  for (int32_t t_old : to_tier3) {
    pprhip_stats_t s1;
    std::memset(&s1, 0, sizeof s1);
    const int32_t t = g->gr->relabeled ? o2n[t_old] : t_old;
    PPRHIP_TRY(c.weighted ? weighted_backward_search_whole(g, t, c.alpha, c.threshold, s1)
                          : backward_search_whole(g, t, c.alpha, c.threshold, s1));
    PPRHIP_CHECK_HIP(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), g->stream));
    PPRHIP_TRY(launch_emit_reserve(g, g->reserve, g->gr->n, c.threshold, t_old, d_rec, cap, d_cnt));
    unsigned long long cnt = 0;
    PPRHIP_CHECK_HIP(hipMemcpyAsync(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, g->stream));
    PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    if (cnt > cap) {
      set_error("All-Pair: a search yields more entries (%llu) than the graph has nodes", cnt);
      return PPRHIP_ERR_STATE;
    }
    if (cnt) PPRHIP_TRY(c.store.take_device(g, d_rec, cnt));
    st.pops += s1.pops + s1.dense_nodes;
    st.edge_pushes += s1.edge_pushes + s1.dense_edges;
    st.levels += s1.levels;
    st.dense_levels += s1.dense_levels;
    st.push_bytes += s1.push_bytes + 16ull * cnt;
  }
  if (c.debug) fprintf(stderr, "[apbs host] whole-vector searches: %zu targets\n", to_tier3.size());
  to_tier3.clear();
  return PPRHIP_OK;
}

// ---- more such searches than that, but fewer than the dense tier ran: once more with a few workspaces whose lists hold
// every node, all the other workgroups helping with their levels; what is left in to_tier3 afterwards gave up there too
int xl_pass(ApbsCall& c, size_t to_tier2_size, std::vector<int32_t>& to_tier3) {
  pprhip_graph* g = c.g;
  const bool run = g->apbs_dense.blocks && !to_tier3.empty() && to_tier3.size() < to_tier2_size && !hook_env("PPRHIP_APBS_NO_XL");
  if (!run) return PPRHIP_OK;
  PPRHIP_TRY(ensure_apbs_workspace(g, g->apbs_xl, 4, 1, g->gr->n + 4096u, g->gr->n + 64u, "full-size"));
  if (!g->apbs_xl.blocks) return PPRHIP_OK;
  use_workspace(c.B, g, g->apbs_xl);
  std::vector<int32_t> again3;
  ApbsDebugRows dbg(c.B, c.debug);
  const int rc = run_tier(c, true, to_tier3, false, again3);
  dbg.print("[apbs dense, full-size pass]", false);
  PPRHIP_TRY(rc);
  if (c.debug) fprintf(stderr, "[apbs host] full-size workspaces: %zu targets, %zu left for tier 3\n", to_tier3.size(), again3.size());
  to_tier3.swap(again3);
  return PPRHIP_OK;
}

// ---- tier 3 (fallback): searches whose frontier outgrows tier 2's lists run as whole-vector backward searches,
// 16 of them in flight on the batch slots; levels that touch a large part of the graph run as batched sweeps over
// the out-CSR
int batch_tier(ApbsCall& c, std::vector<int32_t>& to_tier3, pprhip_stats_t& st3) {
  if (to_tier3.empty()) return PPRHIP_OK;  // Base_Whole_Graph.java:76-92
  pprhip_stats_t& st = c.st;
  std::vector<Triple> tr3;
  BatchJob J;
  J.P = c.g;
  J.kind = QueryKind::kBackward;
  J.srcs = to_tier3.data();
  J.q = (int)to_tier3.size();
  J.alpha = c.alpha;
  J.threshold = c.threshold;
  J.triples = &tr3;
  PPRHIP_TRY(batch_run(c.g, J, &st3));
  PPRHIP_TRY(c.store.take_host(c.g, tr3));
  st.pops += st3.pops;
  st.edge_pushes += st3.edge_pushes;
  st.enqueues += st3.enqueues;
  st.levels += st3.levels;
  st.dense_levels += st3.dense_levels;
  st.push_bytes += st3.push_bytes;
  return PPRHIP_OK;
}

struct PhaseClock {  // wall time since the phase before (PPRHIP_APBS_DEBUG's "[apbs host]" lines)
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  double lap_ms() {
    const auto t1 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t).count();
    t = t1;
    return ms;
  }
};

}  // namespace

// Base_Whole_Graph.java:76-92 for the targets [t_begin, t_end): every backward search's entries >= threshold go to
// `store`.  Tier 1 (LDS tables) -> tier 2 (dense workspaces) -> whole-vector searches; a target that outgrows a tier
// is re-run in the next (kernels_apbs.hip).
// (Rounds 3 and 4 ran tier 1 of the next third of a large range on a side stream beside the dense pass of the third
// before.  LDS searches beside a dense pass slow it down by nearly their own duration, so it saved 5 % when tier 1 was a
// quarter of the job; since tier 1 routes its targets by in-degree it is a seventh of it, and the tiers one after the
// other are as fast or faster - R-MAT 22: 655 against 670 ms, R-MAT 24: 1 894 against 1 910 ms - with one pass of each
// tier instead of three.  The side-by-side form was taken out.)
// weighted: the searches of pprhip_weighted_all_pair_backward - the tiers read the weighted records, and what the dense
// and full-size passes give up runs as whole-vector weighted pushes whatever its number (tier 3's slots are unweighted).
int all_pair_collect(pprhip_graph_t* g, double alpha, double threshold, uint32_t t_begin, uint32_t t_end,
                     TripleStore& store, pprhip_stats_t& st, bool weighted) {
  g->topk_active = false;
  CallTimer tm(g);
  // PPRHIP_APBS_TIER = 2 / 3 starts at a later tier (tests exercise every tier that way)
  const int first_tier = hook_env("PPRHIP_APBS_TIER") ? atoi(hook_env("PPRHIP_APBS_TIER")) : 1;
  ApbsCall c{g, alpha, threshold, t_begin, t_end - t_begin, store, st, hook_env("PPRHIP_APBS_DEBUG") != nullptr, weighted};
  PPRHIP_TRY(c.alloc_buffers());
  PPRHIP_TRY(weighted ? ensure_weighted_in_rec(g) : ensure_in_rec(g));
  // the sweep layout over the out-CSR that the whole-vector searches' dense levels need: built with the handle's other
  // first-use work, not inside a later call's searches
  PPRHIP_TRY(ensure_bwd_layout(g));
  PhaseClock clock;
  std::vector<int32_t> to_tier2, to_tier3;
  if (first_tier <= 1) {
    PPRHIP_TRY(run_tier(c, false, {}, true, to_tier2));
    if (c.debug) fprintf(stderr, "[apbs host] tier 1 (kernel passes + hand-over of entries): %.1f ms\n", clock.lap_ms());
  } else {
    for (uint32_t t = t_begin; t < t_end; ++t) (first_tier == 2 ? to_tier2 : to_tier3).push_back((int32_t)t);
  }
  if (!to_tier2.empty()) {
    PPRHIP_TRY(dense_tier(c, to_tier2, to_tier3));
    st.xl_targets = (uint32_t)to_tier3.size();  // searches that outgrew a workspace's lists
    PPRHIP_TRY(whole_searches(c, to_tier3, false));
    PPRHIP_TRY(xl_pass(c, to_tier2.size(), to_tier3));
  }
  if (c.debug) fprintf(stderr, "[apbs host] tier 2 (%zu targets): %.1f ms\n", to_tier2.size(), clock.lap_ms());
  c.free_buffers();  // (up to 2 GB of records: the batch slots need the room)
  pprhip_stats_t st3;
  std::memset(&st3, 0, sizeof st3);
  const size_t n_tier3 = to_tier3.size();
  if (weighted) {
    PPRHIP_TRY(whole_searches(c, to_tier3, true));
  } else {
    PPRHIP_TRY(batch_tier(c, to_tier3, st3));
  }
  if (c.debug) fprintf(stderr, "[apbs host] tier 3 (%zu targets): %.1f ms\n", n_tier3, clock.lap_ms());
  tm.mark(1);
  tm.finish(st);
  for (int i = 0; i < 8; ++i) {
    st.class_ms[i] += st3.class_ms[i];
    st.class_bytes[i] += st3.class_bytes[i];
    st.class_launches[i] += st3.class_launches[i];
  }
  st.push_ms = CallTimer::ms(g->ev[0], g->ev[1]);
  st.rmax_final = threshold;
  st.rounds = (uint32_t)(to_tier2.size());      // targets that needed the dense tier
  st.dense_nodes = (uint64_t)n_tier3;           // targets that needed the whole-vector path
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip

namespace {

// both entry points: the checks, the searches, the index finalisation
int all_pair_index(pprhip_graph_t* g, double alpha, double threshold, int k, uint32_t t_begin, uint32_t t_end,
                   pprhip_index_t** index_out, pprhip_stats_t* stats, const char* fn, bool weighted) {
  PPRHIP_TRY(check_alpha(alpha, fn));
  PPRHIP_TRY(check_threshold(threshold, fn, "threshold"));
  PPRHIP_TRY(check_graph(g, fn));
  if (weighted) PPRHIP_TRY(need_weights(g, fn));
  if (!index_out || t_begin > t_end || t_end > g->gr->n) {
    set_error("%s: bad target range [%u, %u) for n=%u", fn, t_begin, t_end, g->gr->n);
    return PPRHIP_ERR_INVALID;
  }
  pprhip_stats_t st;
  std::memset(&st, 0, sizeof st);
  // the searches' entries stay in HBM, are put in (source, target) order there, and cross PCIe once, in row order
  TripleStore sink;
  const auto t0 = std::chrono::steady_clock::now();
  // first-use work of the finalisation, beside the searches: the pinned ring the sorted entries are downloaded through
  std::thread pin;
  if (!g->ix_stage) {
    try {
      pin = std::thread([g] {
        if (hipSetDevice(g->gr->device) == hipSuccess) (void)ensure_ring(g);
      });
    } catch (const std::system_error&) {  // (no helper thread: the download pins its ring when it gets there)
    }
  }
  // room for the entries a range of this size usually yields (a dozen per target at the thresholds the thesis uses):
  // the store then does not grow - allocate, copy, free - while the searches run
  if (t_end - t_begin >= (1u << 18)) (void)sink.reserve(g, 12ull * (unsigned long long)(t_end - t_begin));
  const int crc = all_pair_collect(g, alpha, threshold, t_begin, t_end, sink, st, weighted);
  if (pin.joinable()) pin.join();
  PPRHIP_TRY(crc);
  const auto t1 = std::chrono::steady_clock::now();
  try {  // (the index arrays are host allocations of hundreds of megabytes: no exception leaves the C ABI)
    PPRHIP_TRY(index_from_device(g, sink.rec, sink.count, k, 0u, g->gr->n, index_out));
  } catch (const std::exception& e) {
    set_error("%s: index finalisation: %s", fn, e.what());
    return PPRHIP_ERR_OOM;
  }
  if (hook_env("PPRHIP_APBS_DEBUG"))
    fprintf(stderr, "[apbs host] searches + hand-over %.1f ms, index finalisation %.1f ms\n",
            std::chrono::duration<double, std::milli>(t1 - t0).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
  if (stats) *stats = st;
  return PPRHIP_OK;
}

}  // namespace

extern "C" {

int pprhip_all_pair_backward(pprhip_graph_t* g, double alpha, double threshold, int k, uint32_t t_begin, uint32_t t_end,
                             pprhip_index_t** index_out, pprhip_stats_t* stats) {
  return all_pair_index(g, alpha, threshold, k, t_begin, t_end, index_out, stats, "pprhip_all_pair_backward", false);
}

int pprhip_weighted_all_pair_backward(pprhip_graph_t* g, double alpha, double threshold, int k, uint32_t t_begin,
                                      uint32_t t_end, pprhip_index_t** index_out, pprhip_stats_t* stats) {
  return all_pair_index(g, alpha, threshold, k, t_begin, t_end, index_out, stats, "pprhip_weighted_all_pair_backward",
                        true);
}

}  // extern "C"
