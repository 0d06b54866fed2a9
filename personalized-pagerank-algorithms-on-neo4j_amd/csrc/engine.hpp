// engine.hpp — device-resident graph handle and the kernel launchers the drivers call.
#pragma once

#include <atomic>
#include <cstdlib>
#include <vector>

#include "common.hpp"

namespace pprhip {

// Device-side counter block (one per graph handle), mirrored into pinned host memory.
constexpr int kMaxBatch = 8;  // sparse levels launched per host round trip

struct DevCounters {
  unsigned long long hist[16];    // sparse batch: hist[i] = frontier of level i (entries << 36 | edges)
  unsigned long long packed[2];   // dense level / seeding output: entries << 36 | edge total
  double dead[2];                 // dead-end mass waiting to land on the source
  // read once per query, in one copy (read_dead_pops): what the push and the walk phases counted since the reset
  unsigned long long dead_pops;      // pushed nodes with out-degree 0
  unsigned long long walk_steps;     // edges followed by walks
  unsigned long long walks_total;    // walks run
  unsigned long long sources_total;  // residue entries that started walks
  unsigned long long walk_loads;     // load instructions the walk kernel's waves issued ...
  unsigned long long walk_lanes;     // ... and the lanes they carried (64 per load = full waves)
  unsigned long long walks_served;   // walks whose terminal was read from the walk index (k_index_serve)
  unsigned long long share_served;   // walks a batched call's terminal cache answered (k_mc_walk<kWalkShared>) ...
  unsigned long long share_stored;   // ... and walks that ran and left their terminal in it (WalkShare)
  double sum_out;                    // reduction result (the walk plan reads it on the device)
  // walk plan of a phase: sources << 36 | walks, counted by the plan kernel, read by the walk kernel on the device.
  // Three cells used in turn: the plan of phase p counts into cell p % 3 and clears cell (p + 1) % 3, which the walks
  // of phase p - 2 were the last to read (the plan of phase p + 1 may run while the walks of phase p still start).
  unsigned long long mc_plan[3];
  // the residue sum a top-k round's plan was derived from, kept per phase like the cells above: the selection that
  // ends the round hands it to the host in its header (no copy command of its own)
  double plan_sum[3];
  // walks of the latest indexed walk phase that the index does not hold: k_mc_plan<0> zeroes it, k_index_serve counts
  // them, k_mc_walk<kWalkIndexed> returns at once when there are none (a whole-graph plan never runs ahead of the walks before)
  unsigned long long walks_over;
  unsigned long long dhist[8];    // dense batch: dhist[i] = frontier that dense level i of the batch starts from
  int dstate[8];                  // dense batch: sweep state of level i (kGsNone: the level does not run)
};
constexpr int kDenseBatch = 6;  // dense levels of a single query launched per host round trip

// State of a dense sweep ("Gauss-Seidel sweeps").  Rows are cut into `gs_blocks` blocks of equal in-edge
// count, processed one after another; what a row leaves in the *current* contribution array when it is applied decides
// what the later blocks of the same sweep read:
//   kGsJacobi   nothing: every row reads the contributions of the level before (one block is enough);
//   kGsEntry    old + new: first sweep of a long dense phase; later blocks get both, earlier ones have read the old;
//   kGsInPlace  new: the array holds contributions that still have to reach the blocks up to their own;
//   kGsFlush    zero: pending contributions are delivered, the new ones reach nobody yet - after it (as after a Jacobi
//               sweep) every contribution is wholly undelivered again, the only state a sparse level can start from.
enum GsState : int { kGsNone = 0, kGsJacobi = 1, kGsEntry = 2, kGsInPlace = 3, kGsFlush = 4 };

// state of the sweep that follows a sweep of state `prev` which left a frontier of nf nodes / ef edges
__host__ __device__ inline int gs_next_state(int prev, unsigned long long nf, unsigned long long ef,
                                             unsigned long long dense_thresh, unsigned long long gs_thresh) {
  if (nf == 0) return kGsNone;
  const unsigned long long tot = nf + ef;
  if (prev == kGsEntry || prev == kGsInPlace) return tot >= gs_thresh ? kGsInPlace : kGsFlush;  // must be finished
  if (tot < dense_thresh) return kGsNone;                                                      // sparse levels follow
  return tot >= gs_thresh ? kGsEntry : kGsJacobi;
}

// one block of a Gauss-Seidel sweep: row ordinals [j_lo, j_hi), their in-edges [e_lo, e_hi)
struct GsBlock {
  uint32_t j_lo, j_hi;
  unsigned long long e_lo, e_hi;
};

// Edge ranges one launch of the single-query edge kernel walks, as 512-edge chunks in a virtual order: window w holds
// the chunks c_lo[w] + (vc - c_pre[w]) for vc in [c_pre[w], c_pre[w + 1]); edges of a boundary chunk outside
// [e_lo[w], e_hi[w]) count as zero (a neighbouring window or block sums them).
constexpr int kMaxWindows = 16;
struct EdgeWindows {
  uint32_t n;
  uint32_t c_pre[kMaxWindows + 1];
  uint32_t c_lo[kMaxWindows];
  unsigned long long e_lo[kMaxWindows], e_hi[kMaxWindows];
};

// Sliced copy of the in-CSR for the single-query sweep.  A gather of one 8-byte contribution moves a whole 128-byte
// line, and lines that leave L2 come at a fifth of the rate of lines that hit it (tools/micro/gather_rate.hip:
// 55 G/s from a 34 MB table and beyond, 250 G/s from a 4 MB one).  So the in-edges are kept a second time sorted
// by (slice of the source id, row):
// the sweep walks slice after slice, and while a slice is being walked the contributions it gathers - `width`
// consecutive ids, a few MB - stay in every XCD's L2.  A row's edges inside one slice form a *segment*; segment sums
// are added to the row's accumulator (seg_row: segment -> row ordinal), so a row receives one add per slice it has
// sources in.  Built at graph lift when the sources span more than one slice.
struct SlicedLayout {
  int S = 0;                         // slices
  uint32_t width = 0;                // source ids per slice
  int32_t* ci = nullptr;             // [m padded] source ids, slice-major
  uint8_t* flags = nullptr;          // bit e: edge e is the first of its segment
  uint32_t* chunk_starts = nullptr;  // segments that start before each 512-edge chunk
  uint32_t* seg_row = nullptr;       // [segments] row ordinal (index into nz_rows / acc_nz)
  uint32_t n_seg = 0;
  std::vector<uint64_t> edge_base, seg_base;   // [S + 1] first edge / segment of every slice
  std::vector<uint32_t> h_seg_row, h_seg_off;  // host: row ordinal and first edge of every segment
  std::vector<EdgeWindows> plan;               // windows of every Gauss-Seidel block for plan_B blocks
  int plan_B = -1;
};

constexpr int kPanelQueues = 64;  // = the most Gauss-Seidel blocks a sweep can have
// The row-panel copy of the in-CSR on the device (engine_internal.hpp: HostPanelLayout; single-query forward sweep).
struct PanelLayout {
  int32_t* src = nullptr;          // [n_edges] sources, item-major
  uint16_t* rloc = nullptr;        // [n_edges] row ordinal inside the panel (0xffff: padding)
  PanelItem* items = nullptr;      // [n_items]
  PanelDesc* panels = nullptr;     // [n_panels]
  uint32_t n_panels = 0, n_items = 0;
  uint64_t n_part = 0;             // doubles a handle's buffer of the parts' sums holds
  std::vector<uint32_t> h_panel_item0;  // host: [n_panels + 1], the Gauss-Seidel blocks' item windows
};

enum PushMode : int { kFwdWhole = 0, kFwdTopk = 1, kBackward = 2, kPower = 3 };

// Seed table of a query personalized to a weighted node set (seeds.cpp; DESIGN.md §2 "Seed sets").  p is resolved for
// the dead-end seeds: with D = the weight of the dead-end seeds, mass x landing on p gives a live seed i the residue
// x * q_i, q_i = p_i / (1 - (1 - alpha) D), and a dead-end seed j the reserve x * e_j, e_j = alpha p_j / (1 - (1 - alpha) D).
// Arrays in HBM, allocated on first use and grown; freed with the graph.
struct SeedTable {
  uint32_t cap = 0;               // entries id / w / eoff / zin hold
  int32_t* id = nullptr;          // internal ids: the live seeds (ascending), then the dead-end seeds
  double* w = nullptr;            // q_i of a live seed, e_j of a dead-end seed
  uint32_t* eoff = nullptr;       // [n_live] the live seeds' edge offsets as the first frontier list
  int32_t* zin = nullptr;         // [n_zin] live seeds without in-edges (extra rows of the dense apply)
  double* w_node = nullptr;       // [n] q per node, zero elsewhere: the dense apply's landing weights
  unsigned int* done = nullptr;   // workgroups of a landing launch that have read the dead-mass cell
  uint32_t n_live = 0, n_dead = 0, n_zin = 0;
  uint64_t e_live = 0;            // out-edges of the live seeds
  int32_t max_id = -1;            // largest internal id of the set
  std::vector<int32_t> h_id, h_zin;  // host staging of the arrays above
  std::vector<double> h_w;
  std::vector<uint32_t> h_eoff;
};

struct SelRec {  // one candidate of a top-k selection / one entry >= threshold of a backward search
  int32_t id, pad;
  double val;
};
constexpr int kSelHeader = 64;  // bytes before the records in pprhip_graph::sel_blob (kernels_select.hip)

struct PushArgs {
  double alpha;
  double rmax;
  double min_rmax;  // kFwdTopk only
  int32_t src;      // source (forward) or target (backward)
  int mode;
};

// Kernel-class timing with an event pool, resolved after the stream has drained.  Events are
// created on demand and reused across calls; the pool is capped: a call that records more intervals
// than kMaxEvents / 2 (All-Pair's tier 3 launches ~1e5 sparse batches) drains the stream, folds what it
// has into per-class accumulators and starts over, so neither the pool nor `recs` grows with the call.
// Class *times* are an option (pprhip_set_kernel_timing, PPRHIP_KERNEL_TIMER=1): an interval is two event records in
// the stream, and between the short kernels of a top-k round or a sparse level those cost the latency-bound paths
// 2-8 % (round 4: top-k 16 in flight 1 640-1 720 -> 1 800-1 850 queries/s without them).  Without the option the
// brackets are only counted: class_launches and class_bytes are filled, class_ms stay zero.
extern std::atomic<int> g_kernel_timing;  // device_io.cpp; -1: not decided yet (the environment is read on first use)
bool kernel_timing_on();
int kernel_timing_level();  // 0: counted only; 1: every class timed; 2: the dense sweeps (classes 1 and 5) timed only
struct KernelTimer {
  static constexpr size_t kMaxEvents = 4096;
  static constexpr size_t kNoEvent = ~(size_t)0;
  bool off = false;  // records nothing (work whose time is accounted elsewhere or not at all)
  bool last_timed = false;  // the outermost open bracket recorded an event (its end() records the partner)
  int depth = 0;            // brackets open
  std::vector<hipEvent_t> ev;
  struct Rec { int cls; size_t i; uint64_t bytes; };
  std::vector<Rec> recs;
  size_t used = 0;
  hipStream_t stream = nullptr;
  double acc_ms[8] = {0};
  uint64_t acc_bytes[8] = {0};
  uint32_t acc_cnt[8] = {0};
  hipEvent_t next() {
    if (used == ev.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      ev.push_back(e);
    }
    return ev[used++];
  }
  // folds the recorded intervals into the accumulators (the stream must have drained)
  void fold() {
    for (const Rec& r : recs) {
      if (r.i == kNoEvent) {  // counted, not timed
        acc_bytes[r.cls] += r.bytes;
        acc_cnt[r.cls]++;
        continue;
      }
      if (r.i + 1 >= used) continue;
      float f = 0.f;
      if (hipEventElapsedTime(&f, ev[r.i], ev[r.i + 1]) != hipSuccess) continue;
      acc_ms[r.cls] += (double)f;
      acc_bytes[r.cls] += r.bytes;
      acc_cnt[r.cls]++;
    }
    used = 0;
    recs.clear();
  }
  // room for k more intervals without a fold in between (callers that keep indices into `recs`)
  // - in counting mode as well, where begin() folds at kMaxCounted records: a fold between reserve() and the use of
  // an index would let the index name another record
  static constexpr size_t kMaxCounted = 65536;
  void reserve(size_t k) {
    if (off) return;
    if (!kernel_timing_on()) {
      if (recs.size() + k > kMaxCounted) fold();
      return;
    }
    if (used + 2 * k > kMaxEvents && hipStreamSynchronize(stream) == hipSuccess) fold();
  }
  // Brackets on one timer do not nest: a bracket's interval is the pair (begin event, next event).  One opened while
  // another is open - a driver turn taken from inside a wait that a longer bracket spans - is counted, not timed, so
  // the outer pair stays a pair (its time then includes the inner launches: they ran inside it).
  void begin(int cls, uint64_t bytes) {
    if (off) return;
    const bool nested = depth++ > 0;
    const int lvl = kernel_timing_level();
    const bool timed = !nested && (lvl == 1 || (lvl == 2 && (cls == 1 || cls == 5)));  // (PPRHIP_KERNEL_DENSE_PULL / _DENSE_PULL_BATCH)
    if (!nested) last_timed = timed;
    if (!timed) {
      if (recs.size() >= kMaxCounted) {  // (counting needs no drained stream - unless timed brackets are pending too)
        if (used && hipStreamSynchronize(stream) != hipSuccess) return;
        fold();
      }
      recs.push_back({cls, kNoEvent, bytes});
      return;
    }
    if (used + 2 > kMaxEvents) {
      if (hipStreamSynchronize(stream) != hipSuccess) return;
      fold();
    }
    hipEvent_t a = next();
    if (!a) return;
    recs.push_back({cls, used - 1, bytes});
    (void)hipEventRecord(a, stream);
  }
  void end() {
    if (off) return;
    if (depth > 0 && --depth > 0) return;  // (the end of a nested bracket)
    if (!last_timed) return;
    last_timed = false;
    hipEvent_t b = next();
    if (b) (void)hipEventRecord(b, stream);
  }
  // bytes of launches already recorded that only become known later (a walk kernel's steps)
  void add_bytes(int cls, uint64_t bytes) { acc_bytes[cls] += bytes; }
  void reset() {
    used = 0;
    depth = 0;  // (a call that failed between a begin and its end left one open)
    last_timed = false;
    recs.clear();
    for (int c = 0; c < 8; ++c) {
      acc_ms[c] = 0.0;
      acc_bytes[c] = 0;
      acc_cnt[c] = 0;
    }
  }
  // adds everything recorded since reset() to per-class totals (call after the stream has been synchronized)
  void resolve(double tot[8], uint64_t bytes[8], uint32_t cnt[8]) {
    fold();
    for (int c = 0; c < 8; ++c) {
      tot[c] += acc_ms[c];
      bytes[c] += acc_bytes[c];
      cnt[c] += acc_cnt[c];
    }
  }
  void destroy() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear();
    reset();
  }
};

struct BatchSync;  // engine_internal.hpp, batch.cpp: rendezvous of the batch workers at dense levels

// Contribution vector of a dense level: a plain array for a single query (stride 1), or one
// column of the interleaved c8[v][slot] array that kBatch concurrent queries share.
constexpr int kBatch = 16;
struct CView {
  double* p;
  uint32_t stride, off;
  __host__ __device__ double& at(uint32_t v) const { return p[(size_t)v * stride + off]; }
};

// Per-slot arguments of a batched dense level, read by the kernels from device memory.
struct SlotArgs {
  double* res;
  double* reserve;
  uint8_t* flags;
  uint32_t* armed;
  DevCounters* ctr;
  double alpha, rmax, min_rmax;
  int32_t src;
  int32_t active;  // the slot takes part in this sweep
  int32_t mode;
  int32_t dead_slot, out_slot;
  int32_t gs_state;  // GsState of this slot in this sweep
  // a seed-set query (SeedTable of the slot's workspace; seed_w nullptr: not seeded): the live seeds' landing weights
  // per node for the apply kernel, the dead-end seeds (seed_id / seed_e [seed_n_live, seed_n_all)) and the done counter
  // for k_seed_land_dense_batch
  const double* seed_w;
  const int32_t* seed_id;
  const double* seed_e;
  unsigned int* seed_done;
  uint32_t seed_n_live, seed_n_all;
};

// Small results the host waits for (kernels_host.hip): mapped pinned memory a kernel writes and the host reads.
constexpr uint32_t kMailWords = 4112;  // the selection's header and 2048 records fit
struct HostMail {
  unsigned long long seq;  // written last; the host spins on it
  unsigned long long pad[7];
  unsigned long long words[kMailWords];
};

struct ClearList {  // ranges one k_clear launch zeroes
  void* p[6];
  unsigned long long bytes[6];
  int n;
};

// Terminals of the walks (seed, stream 0, v, idx < cap(v)) with the forced first hop at one alpha, per node v, with
// cap(v) = ceil(d_out(v) * density): the table behind the walk index and the call's terminal cache (walk_index.cpp).
struct TerminalTable {
  unsigned long long* off = nullptr;    // [n + 1] first cell of every node, internal order
  int32_t* term = nullptr;              // [total] terminals, internal ids (the cache's kernels take the cells as uint32_t)
  unsigned long long* usage = nullptr;  // counter cells (WalkIndex: 3, WalkShare: 2)
  std::vector<unsigned long long> h_off;
  double alpha = 0.0, density = 0.0;
  uint64_t seed = 0, total = 0;
};

// FORA+ walk index (walk_index.cpp; DESIGN.md §2 "Walk index"): every cell of the table filled by its build.  Lives on
// the lifted graph, read-only after its build; the usage counters are the only cells kernels write: [3] walks served
// from the index / walked live in served phases; the build's walk steps.
struct WalkIndex : TerminalTable {};

// Call-scoped terminal cache of the batched whole-graph FORA paths (walk_index.cpp: walk_share_begin; DESIGN.md §2
// "Walk index", "Terminals shared inside a call").  Every query of a batched call walks with the call's seed and stream
// 0, so walk (v, j) ends at the same terminal whichever query draws it: the first one to walk it leaves the terminal in
// term[off[v] + j] (j < cap(v), the walk index's capacity at the call's density), later ones read it and only deposit.
// A cell is kWalkShareEmpty or the one value every writer would write, so no lock or fence orders readers and writers.
// Owned by the batch state; valid for one (seed, alpha): cleared at the start of every call that uses it.
constexpr uint32_t kWalkShareEmpty = 0xFFFFFFFFu;
constexpr int kWalkShareMinQueries = 32;  // calls of fewer queries run without the cache
// Deposit records of a batched call's walk phases (kernels_walk.hip "deposits by tile"): walk
// gidx < cap of a phase stores (terminal, increment) at position gidx instead of adding at the terminal; the records are
// binned by tile of `1 << tile_shift` consecutive ids, summed per tile in LDS and added to the vector in runs.  The
// records reach their tile's run in two passes that store whole lines: into the run of their coarse bin (`bin`
// consecutive tiles) in bkey/binc, then from there into the tile's run, back in key/inc.  One set per handle: the
// phases that use it run one after another on the batch state's walk stream.  Lives and dies with the call's terminal
// cache (WalkShare), under the same memory rule.
constexpr uint32_t kDepTileShift = 11;     // 2 048 doubles: 16 KB of LDS in the sum kernel
constexpr uint32_t kDepMaxTiles = 4096;    // more tiles than this (16 KB of counters in LDS): the walks keep their atomics
constexpr uint32_t kDepSlice = 16384;      // records of a work item: a hot tile is summed by several workgroups
constexpr unsigned long long kDepMinWalks = 1ull << 18;  // a phase of fewer walks keeps its atomics
constexpr uint32_t kDepBin = 32;           // tiles of a coarse bin: 64 bins on R-MAT 22
constexpr uint32_t kDepMaxBin = 64;        // (a pass sorts into at most kDepMaxBins runs: a counter per thread)
constexpr uint32_t kDepMaxBins = 256;      // more bins than this: the bin grows (4 096 tiles: 16 tiles at the least)
constexpr uint32_t kDepChunk = 2048;       // records a workgroup of a binning pass sorts in LDS at a time (24 KB)
struct DepositArgs {  // what the kernels take, by value
  uint32_t* key = nullptr;   // [cap] terminal of walk gidx (internal id) ...; after the second pass: in per-tile runs
  double* inc = nullptr;     // [cap] ... and what it adds there
  uint32_t* bkey = nullptr;  // [cap] the same records in per-bin runs
  double* binc = nullptr;
  uint32_t* tile_cnt = nullptr;  // [n_tiles] records per tile: counted, turned into items and zeroed again per phase
  uint32_t* tile_cur = nullptr;  // [n_tiles] next free position of every tile's run
  uint32_t* bin_cur = nullptr;   // [n_bins + 1] next free position of every bin's run; [n_bins]: units of the phase
  uint4* items = nullptr;        // [items_cap] {tile, first record, records, the tile has other items}
  uint4* units = nullptr;        // [units_cap] second pass: {bin, first record of the bin's run, records, 0}
  // [0] items of the phase in flight; since the last reset: [1] binned phases, [2] records, [3] walks beyond cap
  unsigned long long* stat = nullptr;
  unsigned long long cap = 0, min_walks = 0;
  uint32_t tile_shift = 0, n_tiles = 0, slice = 0, items_cap = 0, n = 0;
  uint32_t bin = 0, n_bins = 0, units_cap = 0;  // tiles per coarse bin, bins (<= kDepMaxBins)
  // hooks library only (PPRHIP_WALK_DEPOSIT_SKIP): the pass that keeps its loads and arithmetic but stores nothing
  uint32_t skip = 0;
};
enum { kDepSkipNone = 0, kDepSkipCount = 1, kDepSkipScatter = 2, kDepSkipSum = 3 };  // (scatter: both binning passes)
struct WalkDeposit {
  DepositArgs a;
  void* block = nullptr;  // the one allocation behind the arrays
  size_t bytes = 0;
  unsigned long long want = 0;  // the capacity asked for (a.cap: what a quarter of the free memory allowed)
  bool on = false;        // the call's walk phases record (off: atomics, as without the buffers)
};

struct WalkShare : TerminalTable {  // (usage: [2] walks served from the cache / terminals stored, since the last reset)
  hipEvent_t cleared = nullptr;  // recorded behind the clear: the call's walk kernels wait for it
  bool on = false;               // the queries in flight may use it (walk phases of its seed and alpha)
  WalkDeposit dep;               // the deposit records of the call's walk phases, or none
};

// Workspace of the sweep cut (sweep.cpp, kernels_sweep.hip; DESIGN.md §2 "Sweep cut"): allocated by the handle's first
// sweep for all n nodes, kept until pprhip_graph_release(PPRHIP_RELEASE_SWEEP) or the handle's end.
constexpr uint32_t kSweepTile = 4096;        // adjacency slots one workgroup turn of the edge scan covers
constexpr uint32_t kSweepBestBlocks = 1024;  // partial minima of the best-prefix reduction
constexpr int kSweepHdrWords = 8;            // [0] support, [1] best_size, [2] best_cut, [3] best_vol, [4] phi bits, [5] edge slots
                                             // (the weighted sweep: [2] / [3] / [5] in quanta, [6] edge slots)
struct SweepWs {
  unsigned long long* key[2] = {nullptr, nullptr};  // [n] sort keys (inverted score bits), double-buffered
  uint32_t* id[2] = {nullptr, nullptr};             // [n] original ids riding along
  const uint32_t* order = nullptr;                  // the id buffer that holds the order after the sorts
  uint32_t* rank = nullptr;                         // [n] internal id -> position; 0xFFFFFFFF: none
  uint4* rec = nullptr;                             // [n] per position: internal id, out-row begin, out-degree, in-row begin
  unsigned long long* deg = nullptr;                // [n] per position
  unsigned long long* volx = nullptr;               // [n + 1] exclusive vol: volx[i + 1] = vol[i]
  uint32_t* tile_node = nullptr;                    // [tile_cap] first position of every tile of the slot space
  size_t tile_cap = 0;
  long long* delta = nullptr;                       // [n] per position
  unsigned long long* cut = nullptr;                // [n]
  double* part_phi = nullptr;                       // [kSweepBestBlocks]
  unsigned long long* part_idx = nullptr;
  unsigned long long* hdr = nullptr;                // [kSweepHdrWords]
  void* tmp = nullptr;                              // scratch of the library sorts and scans
  size_t tmp_bytes = 0;
  // the weighted sweep alone (weighted_sweep.cpp; allocated by the handle's first weighted sweep): the exclusive vol in
  // quanta, qvolx[i + 1] = vol_q[i].  The positions' qdeg are staged in `cut` until the edge scan's result lands there.
  unsigned long long* qvolx = nullptr;              // [n + 1]
};

// Workspace of the sparse getters (sparse.cpp, kernels_compact.hip; DESIGN.md §2 "Sparse results"): three groups, each
// grown on demand and kept until pprhip_graph_release(PPRHIP_RELEASE_SPARSE) or the handle's end.  A TILE is
// kCompactTile consecutive original ids of one vector; the tiles of a call are numbered vector-major.
constexpr uint32_t kCompactPer = 4;                     // ids a thread takes per tile, 256 apart
constexpr uint32_t kCompactTile = 256u * kCompactPer;   // ids one workgroup covers
struct SparseWs {
  unsigned long long* cnt = nullptr;   // [tile_cap + 1] kept entries per tile, one zero behind the last
  unsigned long long* base = nullptr;  // [tile_cap + 1] their exclusive scan: a tile's first output position; the total
  size_t tile_cap = 0;
  unsigned long long* offs = nullptr;  // [offs_cap] base at every vector's first tile, then the total: the CSR offsets
  size_t offs_cap = 0;
  unsigned long long* val[2] = {nullptr, nullptr};  // [ent_cap] / [sort_cap] value bits of the kept entries
  uint32_t* id = nullptr;                           // [ent_cap] their original ids
  size_t ent_cap = 0;
  unsigned long long* pk[2] = {nullptr, nullptr};   // [sort_cap] by value: vector << 32 | id riding along the sorts
  size_t sort_cap = 0;
  const unsigned long long* val_out = nullptr;      // the value buffer that holds the call's entries in their order
  void* tmp = nullptr;                              // scratch of the library scan and sorts
  size_t tmp_bytes = 0;
};

struct WalkPlanRec {  // one residue entry of a walk phase (k_mc_plan -> k_mc_walk): 32 bytes
  unsigned long long woff;  // walks of the entries before it
  double inc;               // what each of its walks adds at its terminal
  unsigned long long ext;   // the node's out-row (out_ext: first edge | degree << 32)
  int32_t node, orig;       // internal id; original id (a word of the walk's Philox counter)
};

}  // namespace pprhip

namespace pprhip {
namespace detail {
struct FetchPipe;
}

// The lifted graph (pprhip_graph_create): the CSR pair, the internal vertex order and the sweep layouts derived from
// them.  One per handle; the handle and its batch slots reach it through the same pointer (pprhip_graph::gr).  Only the
// lift fills it, plus the builders of the layouts made on first use (gs_blocks_of, sliced_windows_of under a lock,
// ensure_bwd_layout before a batched call's workers start): during a batched call it is read-only.  free_graph_data
// frees it, last of what a handle holds.
struct GraphData {
  int device = 0;
  int n_cus = 256;  // compute units of the device (persistent-kernel grid sizing)
  uint32_t n = 0;
  uint64_t m = 0;
  // CSR pair in HBM: uint32 row pointers, int32 column indices
  uint32_t *out_rp = nullptr, *in_rp = nullptr;
  unsigned long long* out_ext = nullptr;  // per vertex: out row begin | out-degree << 32 (one gather instead of two)
  int32_t *out_ci = nullptr, *in_ci = nullptr;
  uint4* walk_rec = nullptr;  // per out-edge {neighbour, its first out-edge, its out-degree, 0}: one gather per walk step
  std::vector<uint32_t> h_out_rp, h_in_rp;  // host copies for degree checks on the call path
  // internal vertex order: nodes with in-edges first, then by out-degree (descending), so that the contributions the
  // dense sweep gathers most often sit next to each other; the C ABI speaks original ids
  bool relabeled = false;
  int32_t *new2old = nullptr, *old2new = nullptr;
  std::vector<int32_t> h_new2old, h_old2new;
  // dense pull-sweep layout over the in-CSR (in_ci is padded to a multiple of 512 edges)
  uint8_t* start_flags = nullptr;    // bit e: in-edge e is the first of its row
  uint32_t* chunk_starts = nullptr;  // row starts before each 512-edge chunk
  uint32_t n_chunks = 0;
  int32_t* nz_rows = nullptr;  // rows with in-degree > 0, ascending
  uint32_t n_nz = 0;
  std::vector<int32_t> h_nz_rows;  // host copy (block boundaries of the Gauss-Seidel sweeps)
  int32_t* zin_rows = nullptr;     // rows without in-edges
  uint32_t n_zin = 0;
  unsigned long long* cross_bits = nullptr;  // per row ordinal (non-empty rows first): row spans two 512-edge chunks
  uint32_t n_src_live = 0;  // nodes with out-edges: the contributions a forward sweep can gather
  // Internal ids [0, n_live) are the nodes with at least one edge (the vertex order puts nodes with in-edges first, then
  // the others by out-degree: isolated nodes - 43 % of an R-MAT 22 - come last).  A query whose source / target is
  // one of them can only ever hold residue, reserve or walk terminals below n_live, so the passes over "all nodes"
  // (seeding, sums, walk plan, selection, resets) run over n_act = n_live entries; a query on an isolated node uses n.
  uint32_t n_live = 0;
  std::vector<GsBlock> gs_plan;  // blocks of the forward sweep for gs_plan_B blocks (built on demand)
  int gs_plan_B = 0;
  SlicedLayout* sl = nullptr;  // sliced copy of the in-CSR, or none
  PanelLayout* pn = nullptr;   // row-panel copy of the in-CSR, or none
  // the same sweep layout over the out-CSR (backward search: a row pulls from its out-neighbours), built on the first
  // batched backward call
  uint8_t* start_flags_o = nullptr;
  uint32_t* chunk_starts_o = nullptr;
  int32_t *nz_rows_o = nullptr, *z_rows_o = nullptr;  // rows with / without out-edges
  uint32_t n_nz_o = 0, n_z_o = 0;
  unsigned long long* cross_bits_o = nullptr;
  // survival S of the leaking walk at survival_alpha (single pairs, pprhip_walk_survival): internal ids, built on the
  // calling thread before a pair call's workers start, rebuilt only when alpha changes
  double* survival = nullptr;
  double survival_alpha = 0.0;
  WalkIndex* widx = nullptr;  // the walk index, or none (pprhip_walk_index_build / _drop)
  // relationship weights (weighted.cpp: pprhip_graph_set_weights; DESIGN.md §2 "Weighted relationships"), or none:
  // fp64 arrays beside the CSR pair, internal order, read-only after the call.  out_w / out_cum are aligned with
  // out_ci (out_cum: the inclusive left-to-right prefix of each out-row), wsum is W(u), a row's last prefix; in_w is
  // aligned with in_ci and padded like it with 0.0.  24 m + 8 n bytes.
  double *out_w = nullptr, *out_cum = nullptr, *wsum = nullptr, *in_w = nullptr;
  uint64_t w_bytes = 0;  // what the four arrays hold in HBM (0: no weights)
  // survival S_w of the leaking walk over the weighted P at wsurvival_alpha (weighted_bwd.cpp), beside `survival` and
  // not instead of it; goes with the weights (free_weights)
  double* wsurvival = nullptr;
  double wsurvival_alpha = 0.0;
  // the weighted All-Pair searches' in-edge records {source, w / W(source)} (16 B per edge, aligned with in_ci; built on
  // the first pprhip_weighted_all_pair_backward, allpair.cpp); goes with the weights (free_weights) and with
  // PPRHIP_RELEASE_ALL_PAIR.  in_wrec_bytes: what it holds in HBM, counted by pprhip_weights_info while it exists
  void* in_wrec = nullptr;
  uint64_t in_wrec_bytes = 0;
  // the weighted walk index, or none (pprhip_weighted_walk_index_build / _drop): terminals of weighted walks, beside
  // `widx` and never read by the unweighted calls, as `widx` is never read by the weighted ones; built from the weights
  // and dropped before they change (walk_index.cpp: free_weighted_walk_index)
  WalkIndex* widx_w = nullptr;
  // the weighted sweep cut's fixed-point weights (weighted_sweep.cpp; include/pprhip.h "weighted local clustering"):
  // qdeg[v] = the sum of the quanta q(e) over v's out-row and in-row, q_shift the shift s of the quantum rule, q_total
  // the total volume 2 * sum q.  Built by the first weighted sweep after the weights were set, counted by
  // pprhip_weights_info while it exists (qdeg_bytes), gone with the weights (free_weights)
  unsigned long long* qdeg = nullptr;
  int q_shift = 0;
  uint64_t q_total = 0, qdeg_bytes = 0;
};

// The handle's batched-call state: the workspaces ("slots") of its batched queries and the arrays their dense levels
// share - one sweep over the interleaved contribution array c8[v][column] serves every slot waiting at a dense level.
// Built by ensure_batch on the first batched call, destroyed whole by free_batch.
struct BatchState {
  std::vector<pprhip_graph*> slots;
  double* c8[2] = {nullptr, nullptr};
  int c8cur = 0;
  double* acc8 = nullptr;  // [row ordinal][kBatch] row sums
  int acc8_dir = 0;        // layout the row sums were last written in (0 forward, 1 backward)
  unsigned long long* prep_bits = nullptr;  // [kBatch][tiles]: rows holding a contribution after the last sweep
  // what the batched apply kernel needs of a row besides its sums, per row ordinal of a sweep side (0 forward,
  // 1 backward; rows with edges first, then the rows carried behind them): {node, out-degree, in-degree (backward
  // side only, else 0), 0}, padded with node = -1 to apply_meta_rows().  Built on the device from the side's row
  // lists (ensure_apply_meta: the forward side with the batch state, the backward side with its layout).  The fourth
  // word is the class of the row's 64-row tile (ApplyTileClass; the backward side: plain everywhere).
  uint4* apply_meta[2] = {nullptr, nullptr};
  // kBatch SlotArgs, then kApplyListMax tile numbers (the tiles of rows without in-edges a forward sweep visits): one
  // block, one copy per sweep
  SlotArgs* d_slot_args = nullptr;
  SlotArgs* h_slot_args = nullptr;  // pinned
  // Forward sweeps leave the tiles that hold rows without in-edges only alone, except those with the source of a
  // column in the sweep and those of the two sweeps before (DESIGN.md §5 "Rows the apply skips"): the sources' tiles of
  // those two sweeps, and the sweeps that still run over every tile because that history does not say enough (a new
  // batch state, a backward sweep or a seeded column among the last three).  Those sweeps also store the dead-end
  // tiles, on whose rows a backward call's entry preparation may have left a contribution.
  uint32_t zin_hist[2][kBatch];
  int zin_hist_n[2] = {0, 0};
  int zin_full_left = 2;
#ifdef PPRHIP_TEST_HOOKS
  // PPRHIP_APPLY_COUNT_RES, on dead-end tiles: [0] non-zero residues met, [1] residues loaded, [2] tiles an entry sweep
  // came by (take_apply_counts hands them out)
  unsigned long long* apply_res_count = nullptr;
#endif
  unsigned long long* sweep_out = nullptr;    // [kBatch] frontier counters a sweep produced
  unsigned long long* h_sweep_out = nullptr;  // pinned
  unsigned long long* blk_pack8 = nullptr;  // [kBatch][kApplyBlocks8]
  double* blk_dead8 = nullptr;
  uint32_t* blk_ndead8 = nullptr;
  // Workspace pool (batch_driver.hpp: SlotDriver; more workspaces than columns of c8): who holds each column (-1: nobody; an
  // index into `slots`)
  int col_owner[kBatch];
  // Sequential batch driver (SlotDriver): the one stream all slots work on beside the sweeps (sparse levels, seeds,
  // sums, selections), and a stream for the slots' walk phases while sweeps go on (make_side_stream, both)
  hipStream_t slot_stream = nullptr;
  bool slot_stream_tried = false;
  hipStream_t walk_stream = nullptr;
  bool walk_stream_tried = false;
  // called by a slot's small read-backs while they wait (fetch_end): the driver looks after the sweep in flight
  void (*idle_hook)(void*) = nullptr;
  void* idle_arg = nullptr;
  int in_c8 = 0;  // C8Scopes open on the slots (poll_idle: the hook stays out while a slot borrows the sweeps' stream)
  detail::FetchPipe* fetch = nullptr;  // delivery of batched queries' vectors to host memory (engine_internal.hpp)
  WalkShare* share = nullptr;  // terminals the queries of a call share, or none (allocated by the first call that uses it)
};

// A set of All-Pair dense workspaces (allpair.cpp: ensure_apbs_workspace): `blocks` of them in one allocation, their
// lists sized for cap_t popped nodes and a frontier of cap_f; blocks == 0: not there
struct ApbsWorkspace {
  char* ws = nullptr;
  uint32_t blocks = 0, cap_t = 0, cap_f = 0;
};

}  // namespace pprhip

// A graph handle or one of its batch slots: the per-query workspace, the stream it runs on, and the lifted graph it
// borrows.
struct pprhip_graph {
  pprhip::GraphData* gr = nullptr;      // the lifted graph: the handle's own, a slot's parent's
  pprhip::BatchState* batch = nullptr;  // the handle's batched-call state (null until the first batched call and on slots)
  hipStream_t stream = nullptr;
  // single-query dense levels (not on a slot: its dense levels run in the parent's batched sweeps)
  double* acc_nz = nullptr;    // per non-empty row: sum of this level's contributions
  double* pn_part = nullptr;   // [gr->pn->n_part] the items' sums of this handle's panel sweep (first forward dense level)
  uint32_t* pn_ctr = nullptr;  // [kPanelQueues] item queues of a level's edge launches (one per Gauss-Seidel block); k_dense_reduce and reset_query_state zero them
  // batched queries: kBatch workspaces ("slots") borrow this handle's graph and stream; their dense levels run as one
  // sweep over the interleaved contribution array BatchState::c8[v][slot]
  pprhip_graph* parent = nullptr;  // set on a slot
  int slot_index = -1;
  pprhip::BatchSync* sync = nullptr;  // set on a slot while a batched call is running
  hipStream_t own_stream = nullptr;   // slot: the stream its worker thread uses
  // Sequential batch driver (batch_driver.hpp: SlotDriver): a slot's c8-touching kernels go to the parent's stream
  // (engine_internal.hpp: C8Scope), and the events that order them
  bool c8_via_parent = false;
  bool c8_settled = false;  // nothing of this slot is pending on its stream: C8Scope need not wait for that stream
  hipEvent_t c8_ev[2] = {nullptr, nullptr};
  hipEvent_t col_ev = nullptr;  // recorded on the slot's stream when it began to wait for its column
  // Workspace pool (SlotDriver): the slot's index in BatchState::slots; pooled: it has to win a free column - which
  // becomes its slot_index - before it prepares a dense level, and the driver takes the column back when it leaves the
  // sweeps (not pooled: column ws_index % kBatch is its own, as in the threaded driver)
  int ws_index = -1;
  bool pooled = false;
  bool has_col = false;
  uint32_t walk_waves = 0;  // waves per CU of the next walk kernels (0: the default)
  // the last walk phase left records for walks [0, walk_dep_cap) if it had walk_dep_min walks or more (0, 0: atomics;
  // read_dead_pops prices the phase by them)
  unsigned long long walk_dep_cap = 0, walk_dep_min = 0;
  bool stream_open = false;  // a query stream's driver thread owns the handle (stream.cpp: pprhip_stream)
  void* stream_obj = nullptr;  // ... that stream (pprhip_graph_destroy closes a stream its owner forgot)
  hipEvent_t walk_ev[3] = {nullptr, nullptr, nullptr};  // slot: the events around its walk phase on the walk stream
  pprhip::KernelTimer ktimer;  // kernel-class timer of this workspace's work (a slot's worker; a handle's batched sweeps)
  // All-Pair: in-edge records {source, its out-degree} (8 B per edge, built on first use), and tier 2's dense
  // workspaces (16n bytes + lists per workgroup, all-zero between searches), kept between calls: apbs_dense for the
  // workgroups in flight, apbs_xl a few whose lists hold every node, for the searches that outgrow the others
  void* in_rec = nullptr;
  pprhip::ApbsWorkspace apbs_dense, apbs_xl;
  void* apbs_board = nullptr;
  uint32_t apbs_chunk = 0;
  void* ix_stage = nullptr;  // pinned ring the index arrays are downloaded through (index_from_device)
  size_t ix_stage_bytes = 0;
  uint32_t n_act = 0;    // scan bound of the query this workspace is running (0: n; GraphData::n_live)
  uint32_t n_dirty = 0;  // ... of the query before it (what the reset has to clear)
  // per-query state
  double *residue = nullptr, *reserve = nullptr, *est = nullptr;
  double* cdense[2] = {nullptr, nullptr};
  double* cF = nullptr;
  int32_t* F[2] = {nullptr, nullptr};
  uint32_t* eoff[2] = {nullptr, nullptr};
  uint8_t* flags = nullptr;
  // top-k rounds: one bit per node that meets the round's threshold at round start without being parked (possible
  // when the scaled rmax of Fora_Topk.java:133 falls below min_rmax); such a node joins the frontier the first time
  // it receives mass, as Forward_Push.java:226-231 enqueues it, although it does not *cross* the threshold
  uint32_t* armed = nullptr;
  // walk plan
  double sel_plan_sum = 0.0;  // the residue sum the last selection's header carried (select_launch with_plan_sum)
  uint32_t mc_phase = 0;      // walk phases planned since the workspace was reset
  uint32_t mc_last_plan = 0;  // phase of the latest plan: what the next walk kernel runs
  pprhip::WalkPlanRec* mc_plan_rec2 = nullptr;  // second record buffer (odd phases) where plans run ahead of walks
  unsigned long long walk_hint = 0;  // upper bound of the next walk phase's walks when the host knows one (grid size)
  pprhip::WalkPlanRec* mc_plan_rec = nullptr;  // n entries: the residue entries of a walk phase (k_mc_plan)
  // reductions / selection scratch
  double* partial = nullptr;       // 1024 partial sums
  uint32_t sum_np = 0;             // partial sums a launch_sum_partial has left for the walk plan that follows
  uint32_t* hist = nullptr;        // 4096-bin histogram
  unsigned long long* blk_pack = nullptr;  // per-workgroup partial counters of the dense sweep
  double* blk_dead = nullptr;
  uint32_t* blk_ndead = nullptr;
  char* sel_blob = nullptr;        // candidate list: kSelHeader bytes {count, ...} + sel_cap records (SelRec)
  uint32_t sel_cap = 0;
  pprhip::DevCounters* ctr = nullptr;    // device
  pprhip::DevCounters* h_ctr = nullptr;  // pinned host mirror
  pprhip::HostMail* mail = nullptr;      // mapped pinned memory: small read-backs without a copy command (fetch_small)
  pprhip::HostMail* mail_dev = nullptr;  // the same, as the device sees it
  unsigned long long mail_seq = 0;
  // a second stream with its own mail and timer: the next top-k round's push beside this round's walks (fora.cpp:
  // pprhip_fora_topk); created on first use
  hipStream_t spec_stream = nullptr;
  pprhip::HostMail* spec_mail = nullptr;
  pprhip::HostMail* spec_mail_dev = nullptr;
  unsigned long long spec_mail_seq = 0;
  bool spec_failed = false;  // no candidate stream ran beside the compute stream
  hipEvent_t spec_ev[2] = {nullptr, nullptr};  // plan done (compute stream) / speculative push done (second stream)
  pprhip::KernelTimer spec_timer;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  pprhip_tuning_t tun{};
  // resumable top-k push session (Forward_Push object state)
  bool topk_active = false;
  bool topk_first = true;
  int32_t topk_src = -1;
  bool topk_seeded = false;  // the session runs from the seed table (topk_src is -1)
  double topk_alpha = 0.0;
  double topk_rsum = 1.0;
  uint64_t topk_dead_pops = 0;  // DevCounters::dead_pops as the session's last public round read it (it runs since the reset)
  // what `reserve`/`est` currently hold
  bool result_in_est = false;
  // seed-set query in progress (seeds.cpp: SeedScope): dead-end mass lands on the seed table, PushArgs::src is -1
  pprhip::SeedTable* seeds = nullptr;
  bool seed_on = false;
  pprhip::SweepWs* sweep = nullptr;  // the sweep cut's workspace, or none (sweep.cpp)
  pprhip::SparseWs* sparse = nullptr;  // the sparse getters' workspace, or none (sparse.cpp)
};

namespace pprhip {

// ---- kernels_push.hip
// pk0: level 0's frontier (entries << 36 | edges) handed over as an argument; ~0: read it from ctr->hist[0] (a
// compaction kernel wrote it)
int launch_sparse_prepare(pprhip_graph* g, const PushArgs& a, int fbuf, int level, uint64_t nf_upper,
                          unsigned long long dense_thresh, bool scatter_dense, int cbuf, int dead_slot,
                          unsigned long long pk0 = ~0ull);
// levels first .. last of a batch on one workgroup, while they stay below wg_cap entries + edges (k_sparse_levels_wg);
// fbuf0: the list buffer that holds level 0's frontier
int launch_sparse_levels_wg(pprhip_graph* g, const pprhip::PushArgs& a, int fbuf0, int first, int last,
                            unsigned long long dense_thresh, unsigned long long wg_cap, int dead_slot,
                            unsigned long long pk0);
int launch_sparse_push(pprhip_graph* g, const PushArgs& a, int fbuf, int level, uint64_t ef_upper,
                       unsigned long long dense_thresh, int dead_slot, unsigned long long pk0 = ~0ull);
// seed sets (g->seeds): the landing of a sparse level's dead-end mass on p (between the level's two kernels; the dense
// levels land in launch_dense_level)
int launch_seed_land_sparse(pprhip_graph* g, const PushArgs& a, int fbuf, int level, unsigned long long dense_thresh,
                            int dead_slot, unsigned long long pk0);
// Every kernel file has an init_kernels_*: it loads the file's code object and opts the file's own kernels into
// their large dynamic LDS.  Once per device, the thread that lifts the first graph onto it calls them all
// (graph.cpp: init_device_once), so that no launch path sets function attributes or triggers a module load
// later (worker threads launch concurrently).
int init_kernels_push();

// ---- kernels_dense.hip
// One dense level of a single query, block by block (blocks: nullptr / 1 = the whole sweep at once).  state_in:
// device cell holding this level's GsState (a level launched behind another one without a host round trip; kGsNone:
// the kernels return at once), or nullptr: `state0` applies.  hist_out / state_out (nullable) receive the frontier
// the level leaves and the state the level after it has to run in (gs_next_state).
struct DenseLaunch {
  const pprhip::GsBlock* blocks = nullptr;
  int n_blocks = 1;
  const int* state_in = nullptr;
  int state0 = pprhip::kGsJacobi;
  unsigned long long* hist_out = nullptr;
  int* state_out = nullptr;
  unsigned long long dense_thresh = 0, gs_thresh = ~0ull;
};
int launch_dense_level(pprhip_graph* g, const PushArgs& a, int cbuf, int out_slot, int dead_slot,
                       const DenseLaunch& d = DenseLaunch());
namespace detail {
// levels.cpp: the sliced layout's edge windows of every block (nullptr / 1: the whole sweep)
const EdgeWindows* sliced_windows_of(pprhip_graph* g, const GsBlock* blocks, int nb);
}
int init_kernels_dense();

// ---- kernels_dense_batch.hip
constexpr uint32_t kApplyBlocks8 = 2048;  // workgroups of the batched apply kernel (per-slot partials each)
// class of a 64-row tile of the forward side, in the fourth word of its rows' records (k_build_apply_meta).  A mixed
// tile is plain.  Dead end: every row has in-edges and out-degree 0 - it never holds a contribution and, at a dense
// level, never a residue.  No in-edges: every row lies behind the rows with in-edges (or behind the last row).
enum ApplyTileClass : uint32_t { kTilePlain = 0, kTileDeadEnd = 1, kTileNoIn = 2 };
constexpr uint32_t kApplyListMax = 3 * kBatch;  // tiles without in-edges a sweep visits: sixteen sources, three sweeps
static inline size_t slot_args_bytes() { return sizeof(SlotArgs) * kBatch + sizeof(uint32_t) * kApplyListMax; }
// slot arguments already staged in parent->batch->h_slot_args; blocks: Gauss-Seidel blocks (nullptr / 1: one launch)
int launch_dense_level_b8(pprhip_graph* parent, bool backward, const pprhip::GsBlock* blocks = nullptr, int n_blocks = 1);
// records of BatchState::apply_meta for a side of n_rows rows: a trip reads the records of both its tiles without
// asking where the rows end, so the array runs to the end of the tile pair behind the last tile
static inline size_t apply_meta_rows(uint32_t n_rows) { return ((size_t)n_rows / 128 + 2) * 128; }
// fills parent->batch->apply_meta[backward] (allocated, apply_meta_rows records) from the side's row lists
int launch_build_apply_meta(pprhip_graph* parent, bool backward);
#ifdef PPRHIP_TEST_HOOKS
int launch_sweep_edges_only(pprhip_graph* parent, const pprhip::GsBlock& B);
int launch_count_live_lines(pprhip_graph* P, unsigned long long* d_out);
#endif
int init_kernels_dense_batch();

// ---- kernels_frontier.hip
int launch_compact_prepared(pprhip_graph* g, int cbuf, int out_fbuf, unsigned long long* d_counter, bool backward);
int launch_count_active(pprhip_graph* g, const PushArgs& a, int seed_kind, int out_slot);
int launch_seed_list(pprhip_graph* g, const PushArgs& a, int seed_kind, int out_fbuf, unsigned long long* d_counter,
                     bool write_armed = false);
int launch_seed_dense(pprhip_graph* g, const PushArgs& a, int seed_kind, int cbuf, int out_slot, int dead_slot);
int launch_sum(pprhip_graph* g, const double* x, uint32_t n);  // result -> ctr->sum_out
int launch_sum_partial(pprhip_graph* g, const double* x, uint32_t n);  // partial sums -> g->partial, for the plan that follows
bool old_small_kernels();
inline uint32_t act_n(const pprhip_graph* g) { return g->n_act ? g->n_act : g->gr->n; }  // entries a query's passes cover
int launch_set_f64(pprhip_graph* g, double* p, uint32_t idx, double value);
int launch_permute_out(pprhip_graph* g, const double* x, double* out);  // out[old] = x[old2new[old]]
// seed sets (g->seeds): the query's start from p (residue, dead-end reserves, landing weights, and the frontier list
// fbuf - top-k: the parked flags instead), and the landing weights of the set before cleared (its first `count` entries)
int launch_seed_init(pprhip_graph* g, int fbuf, bool topk = false);
int launch_seed_clear(pprhip_graph* g, uint32_t count);
int init_kernels_frontier();

// ---- the other kernel files' init_kernels_* (see init_kernels_push)
int init_kernels_walk();
int init_kernels_select();
int init_kernels_apbs();

// ---- kernels_walk.hip
int launch_build_walk_rec(pprhip_graph* g);
int init_kernels_host();
int launch_publish(pprhip_graph* g, const void* src, uint32_t n_words, unsigned long long seq);
int launch_clear(pprhip_graph* g, const ClearList& L);
int launch_copy_f64(pprhip_graph* g, const double* src, double* dst, size_t n);  // dst[0 .. n) = src[0 .. n), in HBM
int launch_seed_one(pprhip_graph* g, int fbuf, int32_t node);                    // frontier list fbuf = {node}
int launch_hold(hipStream_t stream, unsigned long long ticks);
// The walk phase runs without a host round trip: the plan kernel counts sources and walks into DevCounters::mc_plan
// [g->mc_parity], the walk kernel (a fixed grid) reads them there.  omega_dev > 0: the plan derives rsum and the walk
// budget itself from the residue sum a reduction left in DevCounters::sum_out (top-k rounds: Fora_Topk.java:148-151);
// otherwise rsum / nrw are the host's.
int launch_mc_plan(pprhip_graph* g, int variant, double alpha, double rsum, double nrw, double omega_dev, double* target,
                   const double* copy_src = nullptr, double* copy_dst = nullptr);
int launch_mc_walk(pprhip_graph* g, double alpha, uint64_t seed, uint32_t stream, int no_zero_hop, double* target);
// the walks of the latest plan with the index `ix`: k_index_serve deposits the stored terminals, k_mc_walk<kWalkIndexed> walks
// what the index does not hold (walk idx >= cap of its node, dead-end starts) with the walks' own indices
int launch_mc_walk_indexed(pprhip_graph* g, const TerminalTable* ix, double alpha, uint64_t seed, double* target);
// its first half alone, on a grid the caller sized: k_index_serve reads the plan and the table only, so it serves a
// weighted walk phase from the weighted walk index as well (kernels_weighted.hip: launch_w_walk_run)
int launch_index_serve(pprhip_graph* g, const TerminalTable* ix, double* target, uint32_t grid);
// the walks of the latest plan (whole-graph FORA: stream 0, forced first hop) through the call's terminal cache: a walk
// whose cell is filled deposits there at once, the others walk and fill their cells
// dep: the call's deposit records when this phase may use them (it runs on the walk stream), or null
int launch_mc_walk_shared(pprhip_graph* g, const TerminalTable* ws, double alpha, uint64_t seed, double* target,
                          const WalkDeposit* dep);
// fills ix->term from ix->off (already in HBM): terminal j of node v = walk (seed, stream 0, v, j), forced first hop
int launch_index_build(pprhip_graph* g, const TerminalTable* ix, unsigned long long* d_steps);
// (rows of out-degree >= survival_heavy_degree() go in d_heavy: a workgroup each)
int launch_survival_iter(pprhip_graph* g, const double* s_old, double* s_new, double alpha, const int32_t* d_heavy,
                         uint32_t n_heavy, unsigned long long* dmax);
uint32_t survival_heavy_degree();
int launch_pair_walk(pprhip_graph* g, const int32_t* d_src, uint32_t n_pairs, uint32_t chunks, uint64_t chunk_walks,
                     uint64_t walks, double alpha, uint64_t seed, double* d_part, unsigned long long* d_steps);
int launch_pair_reduce(pprhip_graph* g, const int32_t* d_src, const int32_t* d_pos, uint32_t n_pairs, uint32_t chunks,
                       const double* d_part, uint64_t walks, const double* survival, double* d_values);
int launch_walk_batch(pprhip_graph* g, const int32_t* d_starts, const uint64_t* d_idx, uint64_t count, double alpha,
                      uint64_t seed, uint32_t stream, int no_zero_hop, int32_t* d_term, uint32_t* d_steps);
int launch_mc_pure(pprhip_graph* g, int32_t src, uint64_t n_walks, double alpha, uint64_t seed, double inc,
                   double* target);

// ---- kernels_apbs.hip
// rank that owns source v when [0, n) is cut into `world` contiguous ranges, the first n % world one longer
// (base = n / world, rem = n % world): THE partition rule of the sharded All-Pair - the device partition
// (k_owner_partition), the ranges ranks search (pprhip_shard_target_range) and the host-side partition the CPU
// multi-process tests drive (pprhip_owner_partition) all evaluate this one function
__host__ __device__ inline uint32_t owner_of(uint32_t v, uint32_t base, uint32_t rem) {
  const uint32_t cut = rem * (base + 1u);
  return v < cut ? v / (base + 1u) : rem + (v - cut) / base;
}

struct TripleRec {  // one index entry of All-Pair-Backward-Search on the device: pi(v, t) = p
  int32_t v, t;
  double p;
};
// the control words of one All-Pair launch: 16 words in one allocation (ApbsBuffers::cells), written whole before the
// launch and read back whole after it
enum ApbsCell {
  kApNextTarget = 0,     // target cursor of the large table / the dense tier
  kApOutCount = 1,       // entries the searches wanted to write
  kApOutValid = 2,       // entries below this position are complete (starts at ~0)
  kApOverflowCount = 3,  // length of the list of targets for another pass or the next tier
  kApPops = 4,
  kApEdges = 5,
  kApListLen = 6,        // tier 1 over a range: length of the list of targets with in-edges
  kApSmallCursor = 7,    // ... the small table's target cursor
  kApTargetsDone = 8,    // dense tier: targets finished in this launch
  kApLevelsPosted = 9,   // ... levels that are posted for helpers right now
  kApAbort = 10,         // ... set by a workgroup that waited too long: the launch ends
  kApGiveUpLen = 11,     // tier 1 over a range: length of the small table's give-up list
  kApCells = 16
};
struct ApbsBuffers {
  unsigned long long* cells = nullptr;  // kApCells control words, indexed by ApbsCell
  TripleRec* out_rec = nullptr;  // the searches' entries >= threshold, 16-byte records
  int32_t* overflow = nullptr;
  int32_t *list0 = nullptr, *list1 = nullptr;  // tier 1 over a range: the non-trivial targets, the small table's give-ups
  unsigned long long out_cap = 0;
  char* ws = nullptr;  // tier 2: per-workgroup dense workspaces (owned by the graph handle, see ApbsWorkspace)
  void* board = nullptr;  // tier 2: one entry per workgroup on which it posts a level for helpers (zero at launch)
  uint32_t ws_blocks = 0, cap_t = 0, cap_f = 0, chunk = 0;
  uint32_t helpers = 0;  // tier 2: workgroups a launch may use in all (those beyond ws_blocks only help)
  unsigned long long* dbg = nullptr;  // developer switch PPRHIP_APBS_DEBUG: 12 words per workgroup (kernels_apbs.hip)
};
int launch_owner_partition(pprhip_graph* g, const TripleRec* rec, unsigned long long count, int world,
                           unsigned long long* cursors, TripleRec* out);
size_t apbs_dense_bytes(uint32_t n, unsigned long long m, uint32_t cap_t, uint32_t cap_f, uint32_t chunk);  // one workgroup's tier-2 workspace
uint32_t apbs_default_chunk();
size_t apbs_board_bytes(uint32_t blocks);
int launch_build_in_rec(pprhip_graph* g, void* rec);                  // rec: m records of 8 bytes
int launch_build_in_rec_w(pprhip_graph* g, void* rec);                // rec: m records of 16 bytes, from in_ci / in_w / wsum
// weighted: the searches run over the weighted records (GraphData::in_wrec) instead of the handle's in_rec
int launch_apbs(pprhip_graph* g, bool weighted, bool dense_tier, const int32_t* d_targets, uint32_t t_begin,
                uint32_t n_targets, double alpha, double rmax, ApbsBuffers& b);
// entries >= rmax of a reserve vector (internal ids [0, n)) as records of target t_old; *count counts them all, also
// beyond cap
int launch_emit_reserve(pprhip_graph* g, const double* reserve, uint32_t n, double rmax, int32_t t_old, TripleRec* out,
                        unsigned long long cap, unsigned long long* count);

// ---- kernels_sort.hip
// The index of the rows of sources [v_lo, v_hi) from rec[0 .. count), finished in device memory: rows in the reference's
// order (Base_Whole_Graph.java:112-163: k < 0 target order; k >= 0 entries >= the k-th largest, value descending, ties in
// target order), offsets[n + 1] and the kept entries' targets / values.  count == 0: all three null.  A source outside
// the range or a target outside [0, n) is PPRHIP_ERR_INVALID.  The caller releases the arrays (device_rows_free).
struct DeviceRows {
  unsigned long long* offsets = nullptr;
  int32_t* targets = nullptr;
  double* values = nullptr;
  unsigned long long entries = 0;
};
int finalize_rows_device(pprhip_graph* g, const TripleRec* rec, unsigned long long count, int k, uint32_t v_lo,
                         uint32_t v_hi, DeviceRows* out);
void device_rows_free(DeviceRows* r);
int init_kernels_sort();

// ---- kernels_sweep.hip (the steps of a sweep cut, in launch order; sweep.cpp drives them)
int launch_sweep_support(pprhip_graph* g, SweepWs* w, const double* x, int normalize);  // count -> w->hdr[0]
int launch_sweep_sort(pprhip_graph* g, SweepWs* w, uint32_t count);
int launch_sweep_rank(pprhip_graph* g, SweepWs* w, uint32_t profiled);
int launch_sweep_edges(pprhip_graph* g, SweepWs* w, uint32_t profiled, hipEvent_t before, hipEvent_t after);
int launch_sweep_best(pprhip_graph* g, SweepWs* w, uint32_t profiled, uint64_t max_vol);
// the steps that do not care what the u64 arrays they are given count (the weighted sweep calls them too): a library
// scan, the tiles' first nodes from w->volx, the best prefix over any (exclusive vol, cut) pair and its total volume
int sweep_scan(pprhip_graph* g, SweepWs* w, const unsigned long long* in, unsigned long long* out, uint32_t count);
int launch_sweep_tile_starts(pprhip_graph* g, SweepWs* w, uint32_t profiled);
int launch_sweep_best_over(pprhip_graph* g, SweepWs* w, const unsigned long long* volx, const unsigned long long* cut,
                           uint32_t profiled, uint64_t total_vol, uint64_t max_vol);
// grids under the test switches PPRHIP_SWEEP_ITEM_GRID (workgroups of 256 for `items`, at most cap) / _EDGE_GRID
uint32_t sweep_item_grid(uint64_t items, uint32_t cap);
uint32_t sweep_edge_grid(uint32_t grid);
int init_kernels_sweep();

// ---- kernels_weighted_sweep.hip (the weighted sweep cut's own steps; weighted_sweep.cpp drives them)
// the largest of the m weights, as its bits -> *cell (a zeroed cell; positive doubles order like their bits)
int launch_wsweep_wmax(pprhip_graph* g, unsigned long long* cell);
// qdeg[v] for all n nodes at `shift`, their sum (the total volume in quanta) added to the zeroed *total; the rows of
// kQdegHubRow entries or more go through a list in w->tile_node (two words each) counted in the zeroed *hub_count
constexpr uint32_t kQdegHubRow = 8192;
int launch_wsweep_qdeg(pprhip_graph* g, SweepWs* w, int shift, unsigned long long* qdeg, unsigned long long* total,
                       unsigned long long* hub_count);
int launch_wsweep_support(pprhip_graph* g, SweepWs* w, const double* x, int normalize);  // count -> w->hdr[0]
// launch_sweep_rank with the positions' qdeg beside their count degree: w->volx and w->qvolx
int launch_wsweep_rank(pprhip_graph* g, SweepWs* w, uint32_t profiled);
// launch_sweep_edges adding +q / -q: delta, w->cut (in quanta), w->hdr[6] = edge slots
int launch_wsweep_edges(pprhip_graph* g, SweepWs* w, uint32_t profiled, hipEvent_t before, hipEvent_t after);
int init_kernels_weighted_sweep();

// ---- kernels_compact.hip (ordered stream compaction of result vectors; sparse.cpp drives the steps)
// x: `rows` vectors of n doubles in internal order, one behind the other.  Kept entries: x(v) > threshold.
// tile counts, their scan, the CSR offsets (w->offs[0 .. rows], the last one the total)
int launch_compact_count(pprhip_graph* g, SparseWs* w, const double* x, uint32_t rows, double threshold);
// the kept entries in (vector, id) order: value bits -> w->val[0], ids -> w->id, or (packed) vector << 32 | id -> w->pk[0]
int launch_compact_scatter(pprhip_graph* g, SparseWs* w, const double* x, uint32_t rows, double threshold, bool packed);
// packed entries into (vector, value descending, id ascending) order; ids -> w->id, values -> w->val_out
int launch_compact_sort(pprhip_graph* g, SparseWs* w, uint64_t total, uint32_t rows);
int init_kernels_compact();

// ---- kernels_target.hip (single targets)
// the start of a backward push from a target set: d_id / d_w are `count` distinct internal ids and their weights, padded
// to whole groups of eight entries and 32- / 64-byte aligned; the members over rmax that have in-edges become the
// frontier list fbuf (*d_counter: 0 before, their count << 36 | in-edges after)
int launch_target_init(pprhip_graph* g, const int32_t* d_id, const double* d_w, uint32_t count, int fbuf,
                       unsigned long long* d_counter, double alpha, double rmax);
// g->reserve[v] /= d_survival[v] for v < n, or (lone >= 0) for the entry `lone` alone
int launch_target_finish(pprhip_graph* g, const double* d_survival, uint32_t n, int32_t lone);
int init_kernels_target();

// ---- kernels_weighted.hip (weighted relationships; weighted.cpp drives them, one level per host round trip)
// step 1 of a level that starts from the list fbuf (nf entries): every entry gives up its residue; its per-weight
// contribution c = (1 - alpha) r / W goes to cF[i], or (scatter_dense) to cdense[cbuf][node].  Clears *next_counter.
int launch_w_prepare(pprhip_graph* g, const PushArgs& a, int fbuf, uint32_t nf, bool scatter_dense, int cbuf, int dead_slot,
                     unsigned long long* next_counter);
// step 2 of a sparse level: the list's ef out-edges deposit c * w; the level's dead-end mass lands on a.src; crossings
// are appended to list fbuf ^ 1 and counted into *next_counter (entries << 36 | edges)
int launch_w_push(pprhip_graph* g, const PushArgs& a, int fbuf, uint32_t nf, uint64_t ef, int dead_slot,
                  unsigned long long* next_counter);
// one dense level (a.mode: kFwdWhole, or kPower: every node with mass pops): cdense[cbuf] -> cdense[cbuf ^ 1], the
// frontier it leaves counted into ctr->packed[out_slot], its dead-end mass into ctr->dead[dead_slot ^ 1]
int launch_w_dense_level(pprhip_graph* g, const PushArgs& a, int cbuf, int out_slot, int dead_slot);
int launch_w_walk_batch(pprhip_graph* g, const int32_t* d_starts, const uint64_t* d_idx, uint64_t count, double alpha,
                        uint64_t seed, uint32_t stream, int no_zero_hop, int32_t* d_term, uint32_t* d_steps);
// The weighted walks of the latest plan (launch_mc_plan) on `stream`, with or without the forced first hop
// (pprhip_weighted_fora: 0, forced).  A phase of stream 0 with the forced hop on a handle whose weighted walk index
// (GraphData::widx_w) was built at this alpha, bit for bit, and this seed reads the stored terminals (k_index_serve) and
// walks only what the index does not hold (k_w_walk_plan<true>); every other phase runs k_w_walk_plan<false>.
int launch_w_walk_run(pprhip_graph* g, double alpha, uint64_t seed, double* target, uint32_t stream, bool no_zero_hop);
// fills ix->term from ix->off (already in HBM): terminal j of node v = weighted walk (seed, stream 0, v, j), forced hop
int launch_w_index_build(pprhip_graph* g, const TerminalTable* ix, unsigned long long* d_steps);
int init_kernels_weighted();

// ---- kernels_weighted_query.hip (weighted seed sets and top-k rounds; weighted_query.cpp drives them)
// between the two steps of a sparse level of a seeded push (g->seeds): the level's dead-end mass lands on p - the live
// seeds' residues with the crossing test (crossers join list fbuf ^ 1, counted into *next_counter), the dead-end seeds'
// reserves - and the cell is cleared before launch_w_push looks at it
int launch_wq_land_sparse(pprhip_graph* g, const PushArgs& a, int fbuf, int dead_slot, unsigned long long* next_counter);
// behind a seeded dense apply: the dead-end seeds' share of the level's dead-end mass, and the cell cleared
int launch_wq_land_dense(pprhip_graph* g, int dead_slot);
// a round's first frontier: the nodes active at rmax as list out_fbuf with the prefix of their out-degrees;
// *d_counter: 0 before, entries << 36 | edges after
int launch_wq_collect(pprhip_graph* g, double rmax, int out_fbuf, unsigned long long* d_counter);
int init_kernels_weighted_query();

// ---- kernels_weighted_batch.hip (the dense level of kBatch weighted queries at once; weighted_batch.cpp drives them)
// S: a batch slot whose column of the parent's c8 arrays is slot_index; its kernels run on S->stream.
// launch_w_prepare with the contributions of list fbuf (nf entries) scattered into S's column of c8[c8cur] (all-zero
// before); the list's dead-end mass goes to ctr->dead[dead_slot]
int launch_wbat_scatter(pprhip_graph* S, const PushArgs& a, int fbuf, uint32_t nf, int dead_slot);
// S's column of c8[c8cur] back to list form: F / eoff [out_fbuf] and cF, the column handed back all-zero;
// *d_counter: 0 before, entries << 36 | edges after
int launch_wbat_compact(pprhip_graph* S, int out_fbuf, unsigned long long* d_counter);
// S leaves its column: the rows outside the sweep's rows that its query visits (src: PushArgs::src - the source without
// in-edges, or -1: the live seeds without in-edges of S->seeds) are zeroed in both arrays
int launch_wbat_leave(pprhip_graph* S, int32_t src);
// one batched weighted sweep of the columns staged as active in parent->batch->h_slot_args (res, reserve, ctr, alpha,
// rmax, src, dead_slot, out_slot, seed_w): c8[c8cur] -> c8[c8cur ^ 1], c8cur flipped; an active column's new frontier
// counter goes to its ctr->packed[out_slot] and to sweep_out[column], its next dead-end mass to ctr->dead[dead_slot ^ 1]
int launch_wbat_sweep(pprhip_graph* parent);
// sweep_out[s] = *cells[s] for every non-null cell: the counters of a driver round side by side, for one read-back
int launch_wbat_collect(pprhip_graph* parent, const unsigned long long* const* cells);
int init_kernels_weighted_batch();

// ---- kernels_weighted_topk_batch.hip (the merged walk launch of the batched weighted top-k; weighted_topk_batch.cpp)
struct WalkMultiCol {  // one column of k_w_walk_plan_multi's table (ctr nullptr: idle)
  const WalkPlanRec* plan_rec;  // the column's latest plan
  double* target;               // its estimate
  DevCounters* ctr;
  int cell;                     // the plan's cell: ctr->mc_plan[cell] = sources << 36 | walks
  uint32_t k0, k1;              // the two halves of the column's walk seed
  uint32_t stream;              // ... and its Philox stream (the query's round)
};
// The latest walk plans of the workspaces cols[c] (kBatch entries, nullptr: idle) in ONE launch on the parent's stream:
// column c's walks are (seeds[c], streams[c], node, index) without the forced first hop, added into targets[c]; the
// waves are dealt by walk_multi_deal (weighted_batch.hpp).  Consumes the workspaces' walk hints.
int launch_w_walk_multi(pprhip_graph* parent, pprhip_graph* const* cols, const uint64_t* seeds, const uint32_t* streams,
                        double* const* targets, double alpha);
int init_kernels_weighted_topk_batch();

// ---- kernels_weighted_bwd.hip (the backward direction over the weights; weighted_bwd.cpp drives them)
// step 1 of a backward level that starts from the list fbuf (nf entries): every entry gives up its residue; c =
// (1 - alpha) r goes to cF[i], or (scatter_dense) to cdense[cbuf][node].  Clears *next_counter.
int launch_wb_prepare(pprhip_graph* g, const PushArgs& a, int fbuf, uint32_t nf, bool scatter_dense, int cbuf,
                      unsigned long long* next_counter);
// step 2 of a sparse backward level: the list's ef in-edges (u -> v) deposit (c(v) * w) / W(u) on r(u); crossings are
// appended to list fbuf ^ 1 with their in-degrees and counted into *next_counter (entries << 36 | in-edges)
int launch_wb_push(pprhip_graph* g, const PushArgs& a, int fbuf, uint32_t nf, uint64_t ef, unsigned long long* next_counter);
// one dense backward level over the out-CSR (ensure_bwd_layout first): cdense[cbuf] -> cdense[cbuf ^ 1], the frontier it
// leaves counted into ctr->packed[out_slot]
int launch_wb_dense_level(pprhip_graph* g, const PushArgs& a, int cbuf, int out_slot);
// one Jacobi iteration of the weighted survival (the same edge sweep with x = s_old); dmax: nullptr, or the cell that
// receives max |s_new - s_old| as a bit pattern (zero before)
int launch_wb_survival_iter(pprhip_graph* g, const double* s_old, double* s_new, double alpha, unsigned long long* dmax);
// launch_pair_walk with the weighted walker (chunk sums of g->residue at the terminals -> d_part)
int launch_wb_pair_walk(pprhip_graph* g, const int32_t* d_src, uint32_t n_pairs, uint32_t chunks, uint64_t chunk_walks,
                        uint64_t walks, double alpha, uint64_t seed, double* d_part, unsigned long long* d_steps);
int init_kernels_weighted_bwd();

// ---- kernels_weighted_bwd_batch.hip (the dense level of kBatch weighted backward pushes at once;
// weighted_bwd_batch.cpp drives them)
// S: a batch slot whose column of the parent's c8 arrays is slot_index; its kernels run on S->stream.
// launch_wb_prepare with the contributions of list fbuf (nf entries) scattered into S's column of c8[c8cur] (all-zero
// before)
int launch_wbb_scatter(pprhip_graph* S, const PushArgs& a, int fbuf, uint32_t nf);
// S's column of c8[c8cur] back to list form with the prefix of the in-degrees: F / eoff [out_fbuf] and cF, the column
// handed back all-zero; *d_counter: 0 before, entries << 36 | in-edges after
int launch_wbb_compact(pprhip_graph* S, int out_fbuf, unsigned long long* d_counter);
// behind the first sweep that read a scattered list: the members of list fbuf without out-edges - rows the sweep never
// rewrites - are zeroed in S's column of both arrays
int launch_wbb_leave(pprhip_graph* S, int fbuf, uint32_t nf);
// one batched weighted backward sweep of the columns staged as active in parent->batch->h_slot_args (res, reserve, ctr,
// alpha, rmax, out_slot): c8[c8cur] -> c8[c8cur ^ 1], c8cur flipped; an active column's new frontier counter goes to its
// ctr->packed[out_slot] and to sweep_out[column].  ensure_bwd_layout first; acc8 all-zero in the backward layout.
int launch_wbb_sweep(pprhip_graph* parent);
int init_kernels_weighted_bwd_batch();

// ---- kernels_select.hip
int launch_select_hist(pprhip_graph* g, const double* x, uint32_t n, unsigned long long prefix, int prefix_bits,
                       int digit_bits, bool first_pass);
int launch_select_choose(pprhip_graph* g, unsigned long long k);
int launch_select_gather(pprhip_graph* g, const double* x, uint32_t n, unsigned long long lower_bits, bool zero_count,
                         bool lower_from_device = false, const double* sum_cell = nullptr);

}  // namespace pprhip
