// engine_internal.hpp — declarations shared by the engine's translation units (engine.cpp: single-query
// entry points and the parameter checks; forward_calls.cpp: the forward push, walk-batch and weighted FORA calls;
// graph.cpp: graph lifecycle and workspaces; levels.cpp: level loop; select.cpp: top-k selection;
// device_io.cpp: read-backs, scopes, walk launchers; fora.cpp: resumable FORA / top-k runs; bwd_runs.cpp: the resumable
// runs that push backward; sweep.cpp: sweep cut; sparse.cpp: sparse getters;
// batch.cpp, batch_api.cpp, fetch_pipe.cpp, stream.cpp: the batched entry points; allpair.cpp:
// All-Pair-Backward-Search; index.cpp: its inverted index; pairs.cpp, targets.cpp: single pairs and single targets;
// weighted.cpp: relationship weights, the weighted level loop and power method; weighted_bwd.cpp: the backward
// direction over the weights; weighted_query.cpp: the weighted top-k rounds; weighted_batch.cpp: the batched weighted
// FORA calls; weighted_bwd_batch.cpp: the batched weighted target calls).
#pragma once

#include <sys/mman.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <deque>
#include <string>
#include <vector>

#include "engine.hpp"

// Device-resident result vectors of a batched call (pprhip_results_create): slot i = query i, internal vertex order.
struct pprhip_results {
  pprhip_graph* g = nullptr;
  int device = 0;  // (kept here: the store may be destroyed after its graph)
  int capacity = 0, count = 0;
  double* buf = nullptr;  // capacity x n
};

namespace pprhip {

struct ForaRun;  // run.hpp

// Rendezvous of the batch workers (one host thread and one stream per slot) with the sweeper
// thread.  Workers run their queries' sparse levels, walks and selections concurrently; a worker
// whose next level is dense waits here.  The sweeper runs a batched sweep whenever somebody waits
// and no slot "holds": a slot holds from the moment a sweep releases it until it has said what it
// does next (waits again, goes on with sparse levels, ends its push phase), and while it writes its
// column of the shared contribution array.  Slots busy with sparse levels or walks hold nothing,
// so their kernels overlap the sweeps of the others.
struct BatchSync {
  std::mutex mu;
  std::condition_variable cv;
  pprhip_graph* P = nullptr;
  ForaRun* runs = nullptr;
  int n_wait = 0, n_hold = 0, n_workers = 0;
  bool sweeping = false;
  bool waitflag[kBatch] = {};
  bool hold[kBatch] = {};
  int err = 0;
  std::string errmsg;
  void release(int s);  // the slot stops holding (no-op when it does not)
  void c8_enter(int s);  // before a slot's kernels touch its column of the shared arrays
  int arrive(int s);     // the slot's next level is dense and prepared; returns after the sweep
  void fail(int rc);
  void worker_done(int s);
  void sweeper();
};

}  // namespace pprhip

namespace pprhip {
namespace detail {

struct Triple {  // one index entry of All-Pair-Backward-Search: pi(v, t) = p
  int32_t v, t;
  double p;
};

struct LevelCtx {
  int fcur = 0;   // F/eoff buffer holding the current frontier list
  int ccur = 0;   // dense contribution buffer holding the current level's contributions
  int pslot = 0;  // packed counter slot describing the current frontier
  int dslot = 0;  // dead-mass cell pending for the current level
  uint32_t nf = 0;
  uint64_t ef = 0;
  bool dense_prepared = false;
  int dense_run = 0;  // dense levels run since the current dense phase was seeded
  // Gauss-Seidel sweeps: the state the next dense sweep runs in (set when the level is prepared / yielded), and
  // whether the contribution array is "dirty" (its contributions have reached the later blocks only, so another
  // dense sweep - in place or flushing - has to follow whatever the frontier looks like)
  int gs_state = kGsJacobi;
  bool gs_dirty = false;
  // Batch driver with the slots on a stream of their own (batch_driver.hpp: SlotDriver).  defer_compact: run_levels returns
  // kYieldDefer as soon as the way back to list form is queued (the compaction runs on the parent's stream, before the
  // next sweep; the sparse levels behind it are launched when the driver calls again, beside that sweep).
  // compacted: that compaction has been queued, the list form is (about to be) there.
  bool defer_compact = false;
  bool compacted = false;
  unsigned long long compact_seq = 0;  // mailbox sequence the compaction's end is published under (0: stream order)
};

// FORA rounds that are certain to be followed by another halving do not need their sparse tail: what it
// would push is picked up by the next round's lower threshold.  Such a round ends after the first sparse
// level that follows its dense levels.  fixed: the caller knows another round follows; otherwise the round
// loop's own condition (model cost so far < c_walk * rsum * omega) is evaluated at that point.  The test
// twin applies the same rule (oracle/ppr_oracle.c: round_cut).
struct RoundCut {
  bool enabled = false, fixed = false, had_dense = false, checked = false, taken = false;
  double omega = 0.0, c_walk = 0.0, alpha = 0.0;
  double rsum = 0.0;  // (1 - alpha) * residue sum measured at the check (valid when !fixed and checked)
};

constexpr int kYield = 1;  // run_levels: the next level is dense and the caller runs it (batched sweeps)
constexpr int kYieldColumn = 4;  // run_levels: the level is dense and no column of c8 is free (workspace pool)
constexpr int kYieldDefer = 3;  // run_levels: the compaction is queued, the sparse levels behind it wait for the next call (LevelCtx)
constexpr int kYieldWalk = 2;  // fora_step: the walk phase runs on the handle's side stream; call again when it has ended

// kernel-class timer of the calling thread: its own, or the slot's while it works for a batch
extern thread_local KernelTimer* g_timer_cur;
inline KernelTimer& ktimer() { return *g_timer_cur; }

// Brackets a group of a query's short bookkeeping kernels (class PPRHIP_KERNEL_QUERY_SETUP) for the calling thread's
// timer - when that timer is watching this handle's stream (workspaces are also reset outside any timed call).
// A slot's kernels that touch the shared contribution array c8 (dense prepare, dense seeding, the compaction back to
// list form) while the slot runs on a stream of its own beside the sweeps (c8_via_parent): they go to the parent's
// stream, behind everything the slot has queued so far, and so take their place between two sweeps in stream order.
// back: the slot's stream goes on behind them (the compaction's list is read by the sparse levels); a prepared dense
// level needs no way back - the slot's next work comes after the sweep it waits for has been collected by the host.
struct C8Scope {
  pprhip_graph* g;
  hipStream_t own = nullptr;
  bool on = false, back = false;
  int rc = PPRHIP_OK;
  C8Scope(pprhip_graph* g_, bool back_);
  ~C8Scope() { (void)leave(); }
  int leave();
};

// A slot of the sequential batch driver gives the driver a look at the sweep in flight (BatchState::idle_hook) -
// called between the launches of the slot's longer sequences, which keep the host busy for 100 us and more.
// The hook runs a whole driver turn (collect the sweep, other workspaces' deferred steps, the next sweep) on the
// caller's thread, so it must never be entered while a slot has its stream swapped for the sweeps' (C8Scope): what the
// turn queues for that slot would land on the wrong stream.  No caller does; the counter makes that an invariant the
// code checks instead of one it relies on (SlotDriver::on_idle also refuses to nest, and keeps the sweeps' own timer).
inline void poll_idle(pprhip_graph* g) {
  if (!g->parent) return;
  const BatchState* bs = g->parent->batch;
  if (bs->idle_hook && bs->in_c8 == 0) bs->idle_hook(bs->idle_arg);
}

struct SetupScope {
  KernelTimer* t;
  explicit SetupScope(pprhip_graph* g);
  ~SetupScope() {
    if (t) t->end();
  }
};

// ---- large host arrays that threads fill in full (index arrays, the lift's edge arrays)
inline void* big_alloc(size_t bytes) {
  constexpr size_t kHuge = 2u << 20;
  if (bytes < 8 * kHuge) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p) throw std::bad_alloc();
    return p;
  }
  void* p = nullptr;
  if (posix_memalign(&p, kHuge, (bytes + kHuge - 1) / kHuge * kHuge) != 0 || !p) throw std::bad_alloc();
  (void)madvise(p, (bytes + kHuge - 1) / kHuge * kHuge, MADV_HUGEPAGE);
  return p;
}

// vectors whose resize() leaves new elements uninitialised: the index arrays are hundreds of megabytes that the
// finalisation's threads fill in full (a value-initialising resize is a single-threaded pass over fresh pages)
template <class T>
struct NoInitAlloc {
  using value_type = T;
  NoInitAlloc() = default;
  template <class U>
  NoInitAlloc(const NoInitAlloc<U>&) {}
  // large arrays on 2-MB boundaries with transparent huge pages asked for: the finalisation's threads touch every page
  // of hundreds of megabytes for the first time, and a 4-KB fault each is a fifth of the k rule's time
  T* allocate(size_t n) { return static_cast<T*>(big_alloc(n * sizeof(T))); }
  void deallocate(T* p, size_t) { free(p); }
  template <class U, class... A>
  void construct(U* p, A&&... a) {
    if constexpr (sizeof...(A) == 0) ::new ((void*)p) U;  // default-init: nothing for arithmetic types
    else ::new ((void*)p) U(std::forward<A>(a)...);
  }
  template <class U>
  bool operator==(const NoInitAlloc<U>&) const { return true; }
  template <class U>
  bool operator!=(const NoInitAlloc<U>&) const { return false; }
};
template <class T>
using RawVec = std::vector<T, NoInitAlloc<T>>;


// Row-panel copy of the in-CSR for the single-query forward sweep (round 6).  Why: the sweep gathers one 8-byte
// contribution per in-edge, every gather asks the L1 for a 128-byte line, and a CU keeps ~256 lines in flight
// (TCP_PENDING_STALL_CYCLES: 0.69 of k_dense_edges<true, true>'s cycles; profiles/r06_ell_sweep_study.txt for the model):
// the row-major and the sliced copy ask for 18 M lines per half sweep of R-MAT 22's 33.5 M edges.  Here the rows are cut
// into PANELS of kPanelRows consecutive ordinals whose sums fit half a CU's LDS (64 KB: two workgroups share a CU), and a
// panel's in-edges are sorted by (source, row): neighbouring lanes gather neighbouring sources, so the sources of a line
// are served by one request, and a workgroup walks its part of the contribution array front to back.  R-MAT 22:
// 4.6 M requests to L2 per half sweep where the sliced copy makes 18.1 M (counters: profiles/r06_pmc_single_*.txt).
// A panel of more than kItemEdges edges is cut into S parts of equal edge counts (ITEMS); part k sums into LDS of its own
// and leaves part[base + k * rows + local row]; k_dense_apply adds a row's S values.  Every item's edges are padded to
// whole turns of kPanelStep with (source 0, row 0xffff): a row ordinal no panel has, skipped by the kernel.
struct HostPanelLayout {
  uint32_t n_nz = 0, n_panels = 0, n_items = 0;
  uint64_t n_edges = 0;                      // with padding
  uint64_t n_part = 0;                       // doubles of the parts' sums
  RawVec<int32_t> src;                       // [n_edges] sources, item-major, inside an item sorted by (source, row)
  RawVec<uint16_t> rloc;                     // [n_edges] row ordinal - first ordinal of the panel; 0xffff: padding
  std::vector<PanelItem> items;              // [n_items], panel-major
  std::vector<PanelDesc> panels;             // [n_panels]
  std::vector<uint32_t> panel_item0;         // [n_panels + 1]
};
int build_panel_layout(uint32_t n, uint64_t m, const uint32_t* in_rp, const int32_t* in_ci, const int32_t* nz_rows,
                       uint32_t n_nz, unsigned threads, HostPanelLayout& L);

// The host half of the graph lift (lift.cpp): every array of the internal layout in host memory, ready to upload.
struct HostLift {
  bool relabeled = true;
  std::vector<int32_t> new2old, old2new;
  std::vector<uint32_t> out_rp, in_rp;  // internal order
  RawVec<int32_t> out_ci, in_ci;        // internal order, padded to whole chunks plus one (the padding zeroed)
  std::vector<unsigned long long> ext;  // out-row extent per node: first edge | degree << 32
  std::vector<int32_t> nz_rows, zin_rows;
  uint32_t n_chunks = 0, n_src_live = 0;
  std::vector<uint8_t> flags;
  std::vector<uint32_t> chunk_starts;
  std::vector<unsigned long long> cross;
  // sliced copy of the in-CSR (S == 0: none)
  int S = 0;
  uint32_t width = 0, n_seg = 0;
  std::vector<uint64_t> edge_base, seg_base;
  RawVec<int32_t> sl_ci;
  std::vector<uint8_t> sl_flags;
  std::vector<uint32_t> sl_chunk_starts, seg_row, seg_off;
  // row-panel copy of the in-CSR (n_items == 0: none; graphs that have it have no sliced copy)
  HostPanelLayout pn;
};
// threads: 0 = what the process may use (host_threads)
int lift_host(uint32_t n, uint64_t m, const uint32_t* out_rp, const int32_t* out_ci, const uint32_t* in_rp,
              const int32_t* in_ci, unsigned threads, HostLift& H);
unsigned host_threads();  // CPU affinity and cgroup quota of the process, at most 64 (PPRHIP_HOST_THREADS overrides)

// ---- walk_index.cpp
void free_walk_index(WalkIndex*& slot);  // a walk index of the lifted graph (GraphData::widx / widx_w), if it has one
// the call-scoped terminal cache of the batched whole-graph FORA paths (engine.hpp: WalkShare)
void walk_share_begin(pprhip_graph* P, int q, double alpha, double rmax, double omega, uint64_t seed);
void free_walk_share(BatchState* B);

// ---- sweep.cpp
void free_sweep(pprhip_graph* g);  // the handle's sweep-cut workspace, if it has one
int ensure_sweep(pprhip_graph* g);  // ... allocated when it has none

// ---- weighted_sweep.cpp
void free_weight_quanta(GraphData* D);  // the weighted sweep's qdeg, shift and total volume, if they were built

// ---- sparse.cpp
void free_sparse(pprhip_graph* g);  // the handle's workspace of the sparse getters, if it has one

// ---- weighted.cpp
// the lifted graph's relationship weights (and what was built from them: the weighted survival, the weighted walk
// index), if it has them
void free_weights(GraphData* D);
void free_weighted_in_rec(GraphData* D);  // the weighted All-Pair records alone (PPRHIP_RELEASE_ALL_PAIR)
int need_weights(const pprhip_graph* g, const char* fn);  // PPRHIP_ERR_STATE when the handle has no weights
int fetch_packed(pprhip_graph* g, const unsigned long long* cell, uint32_t* nf, uint64_t* ef);  // a counter cell: entries << 36 | edges
// The level loop of the weighted pushes, forward (kernels_weighted.hip) and backward (a.mode == kBackward:
// kernels_weighted_bwd.hip, no dead-end mass: dslot goes unused): levels from the list L.fcur until the frontier is empty
struct WLevels {
  int fcur = 0, ccur = 0, pslot = 0, dslot = 0;
  uint32_t nf = 0;
  uint64_t ef = 0;
  bool prepared = false;  // the frontier is held as contributions in cdense[ccur] (after a dense level)
};
int run_weighted_levels(pprhip_graph* g, const PushArgs& a, WLevels& L, pprhip_stats_t& st);

// ---- stream.cpp
void stream_detach(void* stream_obj);  // ends a query stream's driver before its graph goes

// ---- graph.cpp
int alloc_dev(void** p, size_t bytes);
int alloc_pinned(void** p, size_t bytes, unsigned flags);  // pinned host memory, zeroed
int reset_query_state(pprhip_graph* g, bool clear_flags, int32_t node = -1);  // node: the query's source / target (internal id)
int ensure_batch(pprhip_graph* P);
void free_batch(pprhip_graph* P);
int ensure_bwd_layout(pprhip_graph* P);
int ensure_panel_part(pprhip_graph* g);  // the buffer of the panel sweep's partial sums (first forward dense level)
int ensure_workspaces(pprhip_graph* P, int count);  // more workspaces than columns of c8 (batch_driver.hpp: SlotDriver)

// ---- levels.cpp
double level_cost(const pprhip_graph* g, uint64_t nf, uint64_t ef, bool* dense);
uint64_t dense_level_bytes(const pprhip_graph* g);
double dense_sweep_cost(const pprhip_graph* g);
uint64_t dense_level_min_bytes(const pprhip_graph* g);  // compulsory bytes of one single-query sweep
uint64_t batch_sweep_min_bytes(const pprhip_graph* P, bool backward, int n_active);  // ... of one batched sweep
void finish_dense(LevelCtx& L, pprhip_stats_t& st, uint64_t level_bytes, uint64_t min_bytes, uint32_t nf_next,
                  uint64_t ef_next);
// one single-query dense level, timed as PPRHIP_KERNEL_DENSE_PULL; first_of_phase: the first level since the seeding
int launch_dense_pull(pprhip_graph* g, const PushArgs& a, int cc, int out, int ds, bool first_of_phase,
                      const DenseLaunch& dl = DenseLaunch());
int run_levels(pprhip_graph* g, const PushArgs& a, LevelCtx& L, pprhip_stats_t& st, double* model_cost,
               bool yield_dense = false, RoundCut* cut = nullptr);
// blocks of the forward Gauss-Seidel sweep for the handle's tuning (nullptr / 1 block when switched off)
const GsBlock* gs_blocks_of(pprhip_graph* g, int* n_blocks);
unsigned long long gs_thresh_of(const pprhip_graph* g);
int seed_single(pprhip_graph* g, LevelCtx& L, int32_t node, uint32_t degree);
int seed_scan(pprhip_graph* g, const PushArgs& a, int seed_kind, LevelCtx& L);

// ---- device_io.cpp
// a stream that runs beside g->stream - and beside `also`, when given - (self-tested)
int make_side_stream(pprhip_graph* g, hipStream_t* out, hipStream_t also = nullptr);
int fetch_small(pprhip_graph* g, const void* dev, void* host, size_t bytes);  // a few words, without a copy command
int fetch_begin(pprhip_graph* g, const void* dev, size_t bytes, unsigned long long* seq_out);  // ... in two halves
int fetch_end(pprhip_graph* g, unsigned long long seq, const void* dev, void* host, size_t bytes);
int device_sum(pprhip_graph* g, const double* x, double* out, uint32_t count = 0);  // count 0: the query's scan bound
int read_dead_pops(pprhip_graph* g, pprhip_stats_t& st);
int run_walk_phase(pprhip_graph* g, int variant, double alpha, double rsum, long long nrw, uint64_t seed, uint32_t stream,
                   double* target, pprhip_stats_t& st, double omega_dev = 0.0);
int launch_walk_plan(pprhip_graph* g, int variant, double alpha, double rsum, long long nrw, double* target, double omega_dev,
                     const double* copy_src = nullptr, double* copy_dst = nullptr);
int launch_walk_run(pprhip_graph* g, int variant, double alpha, uint64_t seed, uint32_t stream, double* target);

// ---- select.cpp
int select_launch(pprhip_graph* g, const double* x, int k, unsigned long long* seq_out, bool with_plan_sum = false);
int select_finish(pprhip_graph* g, unsigned long long seq, const double* x, int k, int32_t* ids_out, double* vals_out,
                  int cap, int* n_out, double* kth_out, bool* have_kth, pprhip_stats_t& st);
int select_topk(pprhip_graph* g, const double* x, int k, int32_t* ids_out, double* vals_out, int cap, int* n_out,
                double* kth_out, bool* have_kth, pprhip_stats_t& st, bool with_plan_sum = false);

// ---- engine.cpp
int copy_out(pprhip_graph* g, const double* dev, double* host);
int check_graph(const pprhip_graph* g, const char* fn);
inline bool node_in_range(const pprhip_graph* g, int32_t v) { return v >= 0 && (uint32_t)v < g->gr->n; }
int check_node(const pprhip_graph* g, int32_t v, const char* fn);  // PPRHIP_ERR_INVALID unless node_in_range
// parameter ranges (include/pprhip.h): alpha in (0, 1); eps, delta, pfail finite and > 0; thresholds finite and >= 0
int check_alpha(double alpha, const char* fn, const char* name = "alpha");
int check_positive(double v, const char* fn, const char* name);
int check_threshold(double v, const char* fn, const char* name);
int check_conf(const pprhip_fora_conf_t* c, const char* fn, bool topk);
// what every FORA top-k entry point asks of its conf, eps and output row (the message, "fn: bad arguments", is set)
bool topk_args_ok(const pprhip_fora_conf_t* conf, double eps, int cap, const int32_t* ids_out, const double* vals_out,
                  const char* fn);
// q sets described like a CSR: offsets[0] = 0, ascending, no set of more than INT32_MAX members (the message names the set)
int check_set_offsets(const uint64_t* offsets, int q, const char* fn);
// a batched call's result store (NULL: none) belongs to the call's graph and holds its q queries
int check_keep(const pprhip_results* keep, const pprhip_graph* g, int q, const char* fn);
// The caller's ids / weights (NULL: uniform) / count as a weighted set of `noun`s ("seed", "target"): distinct original
// ids ascending and their weights, duplicates summed, zero weights dropped - divided by the sum of all weights with
// `normalize`, as given without.  PPRHIP_ERR_INVALID for an empty set, an id outside [0, n), a negative or non-finite
// weight, or weights that sum to 0; set >= 0: the messages name it ("fn: set N: ...").  `out` is the parser's only
// buffer: a caller with many sets passes the same one again.
using WeightedSet = std::vector<std::pair<int32_t, double>>;
int parse_weighted_set(uint32_t n, const int32_t* ids_in, const double* weights, int k, bool normalize, const char* noun,
                       const char* fn, int set, WeightedSet& out);
uint32_t hdeg_out(const pprhip_graph* g, int32_t v);
uint32_t hdeg_in(const pprhip_graph* g, int32_t v);

// per-class kernel totals into a call's stats; the class with the largest total is the dominant one
inline void fold_class_totals(pprhip_stats_t& st, const double tot[8], const uint64_t bytes[8], const uint32_t cnt[8]) {
  int best = 0;
  for (int c = 0; c < 8; ++c) {
    st.class_ms[c] = tot[c];
    st.class_bytes[c] = bytes[c];
    st.class_launches[c] = cnt[c];
    if (tot[c] > tot[best]) best = c;
  }
  st.dominant_kernel_id = (uint32_t)best;
  st.dominant_kernel_ms = tot[best];
  st.dominant_kernel_bytes = bytes[best];
  st.dominant_kernel_launches = cnt[best];
}

inline double host_ms() {  // the host's steady clock
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct CallTimer {
  pprhip_graph* g;
  explicit CallTimer(pprhip_graph* g_) : g(g_) {
    ktimer().stream = g->stream;
    ktimer().reset();
    (void)hipEventRecord(g->ev[0], g->stream);
  }
  void mark(int i) { (void)hipEventRecord(g->ev[i], g->stream); }
  static double ms(hipEvent_t a, hipEvent_t b) {
    float f = 0.f;
    if (hipEventElapsedTime(&f, a, b) != hipSuccess) return 0.0;
    return (double)f;
  }
  // resolves per-class kernel times; picks the class with the largest total as dominant
  void finish(pprhip_stats_t& st) {
    (void)hipEventRecord(g->ev[5], g->stream);
    (void)hipStreamSynchronize(g->stream);
    st.total_ms = ms(g->ev[0], g->ev[5]);
    double tot[8] = {0};
    uint64_t bytes[8] = {0};
    uint32_t cnt[8] = {0};
    ktimer().resolve(tot, bytes, cnt);
    fold_class_totals(st, tot, bytes, cnt);
  }
};

// Delivery of the queries' vectors to the caller's (pageable) host memory while the batch keeps running: a finished
// query's vector is permuted to the caller's ids into one of kRing device staging buffers on the query's own stream,
// copied to a pinned host buffer on a copy stream, and moved from there to its destination by a copier thread.  The
// compute stream never waits for PCIe or for the host copy; a query that finishes while all staging buffers are in
// flight waits for one.
struct FetchPipe {
  static constexpr int kRing = 16;   // one per slot: the queries of a batch tend to finish in bursts (they leave the shared sweeps together)
  static constexpr int kCopiers = 6;
  pprhip_graph* P = nullptr;
  size_t n = 0;
  hipStream_t cs = nullptr;
  double* dev[kRing] = {};
  double* pin[kRing] = {};
  hipEvent_t ready[kRing] = {};
  hipEvent_t done[kRing] = {};
  struct Item { int e; double* dst; };
  struct Arrival { FetchPipe* pipe; Item item; };
  static void on_copied(void* arrival);  // host callback of the copy stream
  int pending = 0;                       // copies queued on the copy stream whose callback has not run yet
  std::mutex mu;     // free_q, work, pending, closing, err: bookkeeping only - never held across a HIP call, because
                     // the copy stream's host callback (on_copied, on a runtime thread) takes it too
  std::mutex cs_mu;  // orders the slots' threads on the shared copy stream (wait - copy - callback stay together)
  std::condition_variable cv;
  std::deque<int> free_q;
  std::deque<Item> work;
  bool closing = false;
  int err = 0;
  std::thread copiers[kCopiers];
  int ensure(pprhip_graph* parent);  // buffers, stream and events: allocated once per handle, kept between calls
  void start();                      // a call's copier threads
  int submit(pprhip_graph* S, const double* dev_vec, double* dst);  // dev_vec in internal order, on S->stream
  int finish();                      // drains and joins; first error of any stage
  void destroy();
  void copier();
};

// A pair call (pairs.cpp: pair_plan / pair_upload / pair_collect): the pairs sorted by target; the i-th distinct target
// covers the sorted pairs [first[i], first[i + 1]) - query i of a BatchJob kind kPairs (BatchJob::srcs = distinct).
// Device arrays of the call, one block the plan owns: the sources (internal ids) and the call positions of the sorted
// pairs, the values by call position, the steps counter, per workspace a buffer of part_cap chunk sums; and per
// workspace (ws_index < kBatch) of the batched call three events (push start, walks start, end).
struct PairPlan {
  std::vector<uint32_t> first;
  std::vector<int32_t> distinct;      // the distinct targets, ascending (original ids)
  std::vector<int32_t> h_src, order;  // the host halves of d_src / d_pos
  const int32_t* d_src = nullptr;
  const int32_t* d_pos = nullptr;
  double* d_values = nullptr;
  double* d_part = nullptr;  // [workspaces][part_cap]
  size_t part_cap = 0;
  unsigned long long* d_steps = nullptr;  // walk steps of the call
  uint64_t walks = 0;       // w per pair
  uint32_t chunks = 0;      // work items per pair ...
  uint64_t chunk_walks = 0; // ... of this many walks (the last one shorter)
  uint32_t block_pairs = 0; // pairs per walk launch (part_cap / chunks)
  double alpha = 0.0, rmax = 0.0, omega = 0.0;
  uint64_t seed = 0;
  const double* survival = nullptr;
  double t0 = 0.0;  // host clock when the call began its work (ms)
  char* blob = nullptr;
  hipEvent_t ev[3 * kBatch] = {};
  int n_ev = 0;
  PairPlan() = default;
  PairPlan(const PairPlan&) = delete;
  PairPlan& operator=(const PairPlan&) = delete;
  ~PairPlan() {
    for (int e = 0; e < n_ev; ++e) (void)hipEventDestroy(ev[e]);
    if (blob) (void)hipFree(blob);
  }
};

// A single-target call (targets.cpp: target_plan): query i is the backward push from set i of the table -
// members [first[i], first[i + 1]) of d_id / d_w (distinct internal ids, duplicates summed, zero weights dropped; every
// set starts on a multiple of eight entries and is padded to one, kernels_target.hip) - and the division by S.
// single[i]: one member of weight 1, started the pair call's way (r(t) = 1, t popped).  nf / ef: the first frontier of
// a set as k_target_init lists it (members with in-edges over rmax, their in-edges), known to the host beforehand.
// d_id / d_w lie in one device block that the plan owns.
struct TargetPlan {
  std::vector<uint64_t> first;
  std::vector<uint32_t> count, nf;
  std::vector<uint64_t> ef;
  std::vector<int32_t> single;   // the internal id of a single target, else -1
  std::vector<int32_t> max_id;   // largest internal id of the set (the scan bound, reset_query_state)
  const int32_t* d_id = nullptr;
  const double* d_w = nullptr;
  double alpha = 0.0, rmax = 0.0;
  const double* survival = nullptr;
  char* blob = nullptr;
  TargetPlan() = default;
  TargetPlan(const TargetPlan&) = delete;
  TargetPlan& operator=(const TargetPlan&) = delete;
  ~TargetPlan() {
    if (blob) (void)hipFree(blob);
  }
};

// What a query of a batched job runs: whole-graph FORA, FORA top-k (seed + query index), a backward search of
// All-Pair, single pairs (a backward push per distinct target, then its sources' walks), or a single-target query (a
// backward push from a target set, scaled by the survival vector)
enum class QueryKind : int { kFora, kTopk, kBackward, kPairs, kTargets };
inline bool is_whole_graph(QueryKind k) { return k == QueryKind::kFora; }
inline bool pushes_backward(QueryKind k) {
  return k == QueryKind::kBackward || k == QueryKind::kPairs || k == QueryKind::kTargets;
}

// a batch of queries for the slot engine (batch.cpp)
struct BatchJob {
  pprhip_graph* P = nullptr;
  const int32_t* srcs = nullptr;  // nullptr: a job of seed sets (sets) or of target sets (targets)
  int q = 0;
  double eps = 0.0;
  const pprhip_fora_conf_t* conf = nullptr;
  uint64_t seed = 0;
  int n_rounds = 0;
  double* reserve_out = nullptr;
  int k = 0;
  int32_t* ids_out = nullptr;
  double* vals_out = nullptr;
  int* n_out = nullptr;
  pprhip_stats_t* per_query = nullptr;
  QueryKind kind = QueryKind::kFora;
  PairPlan* pairs = nullptr;               // kPairs
  TargetPlan* targets = nullptr;           // kTargets (srcs is nullptr: the plan holds the sets)
  double alpha = 0.0, threshold = 0.0;   // kBackward
  std::vector<Triple>* triples = nullptr;  // kBackward: every search's entries >= threshold
  pprhip_results* keep = nullptr;          // kFora: device-resident store of the queries' vectors
  int keep_first = 0;                      // ... query i goes to slot keep_first + i of it
  FetchPipe* pipe = nullptr;               // reserve_out given: asynchronous delivery (batch_run opens / closes it)
  // kFora and kTopk without srcs: query i runs from seed set i, its host plan (seed_plan) made before anything runs; the
  // query's workspace takes it over (seed_upload) when the query begins
  std::vector<SeedTable> sets;
  pprhip_stats_t sum{};
  std::mutex sum_mu;
  std::atomic<int> next_query{0};
};

// ---- pairs.cpp
int ensure_survival(pprhip_graph* g, double alpha);  // S at alpha on the lifted graph (GraphData::survival), cached per alpha
// The Jacobi iteration behind both survival vectors: from S0 = alpha, double-buffered, on the handle's stream, checked
// every eighth iteration, until (1 - alpha) / alpha * max|dS| <= 1e-14 (the iteration contracts by 1 - alpha).  iter
// queues one iteration s_old -> s_new; its third argument is nullptr or the zeroed cell that receives max|dS| as a bit
// pattern.  both: S0 goes to both buffers (an iteration that leaves some rows unwritten); converged: nothing to
// iterate.  *out: the vector, the caller's to free.  fn names the entry point in the messages.
int survival_jacobi(pprhip_graph* g, double alpha, const char* fn, bool both, bool converged,
                    const std::function<int(const double*, double*, unsigned long long*)>& iter, double** out);
// The front of pprhip_ppr_pairs and pprhip_weighted_ppr_pairs (fn; weighted: the handle must have weights).
// pair_plan: the checks in the documented order, r_max / w / omega, the stats_sum prologue, and for q > 0 the pairs
// grouped by target and the chunk geometry.  pair_upload: the device block with `workspaces` buffers of chunk sums and
// n_events events.  pair_collect: values and steps back to the host, stats_sum filled from sum.
int pair_plan(pprhip_graph_t* g, const int32_t* sources, const int32_t* targets, int q, double eps,
              const pprhip_fora_conf_t* conf, double rmax, uint64_t seed, const double* values_out,
              pprhip_stats_t* stats_sum, const char* fn, bool weighted, PairPlan& pp);
int pair_upload(pprhip_graph* g, PairPlan& pp, int workspaces, int n_events, const char* fn);
int pair_collect(pprhip_graph* g, const PairPlan& pp, double* values_out, pprhip_stats_t& sum, pprhip_stats_t* stats_sum,
                 const char* fn);

// ---- targets.cpp
// The front of pprhip_ppr_targets and pprhip_weighted_ppr_targets (fn; weighted: the handle must have weights): the
// checks in the documented order, the stats_sum prologue, an empty call's keep->count = 0, and for q > 0 the set table
// in tp, its ids and weights uploaded.  The caller returns at once when q == 0.
int target_plan(pprhip_graph_t* g, const int32_t* targets, const double* weights, const uint64_t* offsets, int q,
                double alpha, double rmax, pprhip_results* keep, int k, const int32_t* ids_out, const double* vals_out,
                pprhip_stats_t* stats_sum, const char* fn, bool weighted, TargetPlan& tp);

// ---- batch.cpp
int batch_run(pprhip_graph_t* g, BatchJob& J, pprhip_stats_t* stats_sum);
// delivery of query r.query of J, finished on the workspace r.g with the statistics r.st: the vector into the result
// store and / or the caller's array, the top-J.k selection, the per-query statistics
int deliver_vector(BatchJob& J, ForaRun& r);

// ---- weighted_bwd_batch.cpp
// pprhip_weighted_ppr_targets for q >= 2 behind its checks: the plan's sets (tp.survival = S_w) with up to kBatch in
// flight on the handle's batch workspaces (built on first use), delivered as the serial path delivers them
int weighted_targets_batch(pprhip_graph_t* g, const TargetPlan& tp, int q, pprhip_results* keep, double* values_out, int k,
                           int32_t* ids_out, double* vals_out, int* n_out, pprhip_stats_t* per_query,
                           pprhip_stats_t* stats_sum);

// ---- forward_calls.cpp
int check_weighted_fora_params(double eps, const pprhip_fora_conf_t* conf, double rmax, const char* fn);
#ifdef PPRHIP_TEST_HOOKS
int take_apply_counts(pprhip_graph* g, pprhip_stats_t& sum);  // batch.cpp
#endif

// ---- allpair.cpp
// where the entries of All-Pair's backward searches go: an HBM record store, which the single-GPU call hands to the index
// finalisation and the sharded call partitions by owner of the source and exchanges over RCCL before anything crosses PCIe
struct TripleStore {
  TripleRec* rec = nullptr;
  unsigned long long count = 0, cap = 0;
  ~TripleStore();
  int reserve(pprhip_graph* g, unsigned long long extra);
  int take_device(pprhip_graph* g, const TripleRec* d_rec, unsigned long long count);
  int take_host(pprhip_graph* g, std::vector<Triple>& more);
};
// the searches of the targets [t_begin, t_end), tier by tier; their entries >= threshold are added to `store`
int all_pair_collect(pprhip_graph_t* g, double alpha, double threshold, uint32_t t_begin, uint32_t t_end,
                     TripleStore& store, pprhip_stats_t& st, bool weighted = false);
// Backward_Search.backward_search_whole_graph on the handle's own vectors (internal id); reserve / residue stay in HBM
// (engine.cpp)
int backward_search_whole(pprhip_graph_t* g, int32_t target_internal, double alpha, double rmax, pprhip_stats_t& st);
// ... and its weighted form: pprhip_weighted_backward_push's search (weighted_bwd.cpp)
int weighted_backward_search_whole(pprhip_graph_t* g, int32_t target_internal, double alpha, double rmax,
                                   pprhip_stats_t& st);

// ---- bwd_runs.cpp
// The start of every backward push from one target (internal id), on a workspace the caller has just reset: a and L for
// run_levels, r(t) = 1 and t as the first frontier.  A target without in-edges gets reserve(t) = lone_value instead and
// no push (*pushing false).  lone_value, the one deliberate difference between the callers: 1.0 for All-Pair's searches
// and pprhip_backward_push, which is what Backward_Search.java:46-49 writes; alpha for pairs and targets, which is what
// the standard start (r(t) = 1, t popped) leaves there - p_t(t) = alpha and no residue.
int backward_start(pprhip_graph* g, LevelCtx& L, PushArgs& a, int32_t target_internal, double alpha, double rmax,
                   double lone_value, bool* pushing);
// The walks and values of the sorted pairs [lo, hi) of one target after its push, in blocks of the plan's pairs per
// launch.  part: the workspace's chunk sums; lone: the target has no in-edges, so it left no residue and its values
// are exact without walks; walk: launch_pair_walk or launch_wb_pair_walk.  Counts the walks into st.
int pair_walk_blocks(pprhip_graph* g, const PairPlan& pp, uint32_t lo, uint32_t hi, double* part, bool lone,
                     decltype(&launch_pair_walk) walk, pprhip_stats_t& st);

// ---- index.cpp
// the index over all n sources from entries on the host: bucketed by source, row order and k rule on the host's threads
int index_from_triples(uint32_t n, std::vector<Triple>& tr, int k, pprhip_index_t** out);
// the same from records in HBM: row order and k rule on the device (kernels_sort.hip), the index arrays downloaded as
// they are; sources must lie in [v_lo, v_hi)
int index_from_device(pprhip_graph* g, const TripleRec* rec, unsigned long long count, int k, uint32_t v_lo, uint32_t v_hi,
                      pprhip_index_t** out);
int index_concat(const std::vector<pprhip_index_t*>& parts, pprhip_index_t** out);
int ensure_ring(pprhip_graph* g);  // the pinned ring index_from_device downloads through (g->ix_stage), on first use

// ---- seed sets (seeds.cpp)
// the caller's seeds / weights / count as p (parse_weighted_set for seeds, normalized; set: as there), resolved for the
// dead-end seeds under alpha into the host half of a seed table (h_* arrays and counts)
int seed_plan(pprhip_graph* g, const int32_t* seeds, const double* weights, int k, double alpha, const char* fn,
              SeedTable& plan, int set = -1);
// q seed sets described like a CSR (set i = seeds / weights [offsets[i], offsets[i + 1])) as q plans: the checks of
// parse_weighted_set for every set (the message names the set); bad offsets and q < 0 are PPRHIP_ERR_INVALID as well.
// Host only.
int seed_plan_sets(pprhip_graph* g, const int32_t* seeds, const double* weights, const uint64_t* offsets, int q,
                   double alpha, const char* fn, std::vector<SeedTable>& plans);
int seed_upload(pprhip_graph* g, SeedTable& plan);  // plan -> g->seeds (HBM; allocated on first use, grown)
int seed_start(pprhip_graph* g, LevelCtx& L);       // r = p resolved, the live seeds as L's frontier
int seed_start(pprhip_graph* g, WLevels& L);        // ... of a weighted push
void seed_free(pprhip_graph* g);
// the push levels of the calling query land dead-end mass on the seed table while the scope lasts
struct SeedScope {
  pprhip_graph* g;
  bool on;
  explicit SeedScope(pprhip_graph* g_, bool on_ = true) : g(g_), on(on_) {
    if (on) g->seed_on = true;
  }
  ~SeedScope() {
    if (on) g->seed_on = false;
  }
};

// ---- engine.cpp: the top-k push session (Forward_Push.forward_push_topk, resumed round after round by Fora_Topk)
// a new session from one source (internal id src; Q = {s} parked) or from a seed table (plan; src is ignored), its
// residue sum rsum until a round has measured one
int topk_session_reset(pprhip_graph* g, int32_t src, SeedTable* plan, double alpha, double rsum);
// a round's push at rmax up to its levels: the dead-source rule (Forward_Push.java:149-153; *pushing false, nothing
// to run), the session's first residue, and the scan of the start set into a / L; run_levels(g, a, L, ...) follows.
// A seed-set session runs it and its levels under SeedScope.
int topk_push_start(pprhip_graph* g, double min_rmax, double rmax, PushArgs& a, LevelCtx& L, bool* pushing);

}  // namespace detail
}  // namespace pprhip
