// kernels_dense.hip — the dense level of a single query for gfx950 (MI355X); the other shape: kernels_push.hip.
//
//   dense   k_dense_edges + k_dense_apply + k_dense_reduce: a pull sweep over the non-empty rows of
//           the in-CSR.  Every wave owns 512 consecutive in-edges (8 per lane: two 16-byte column
//           index loads, 8 contribution gathers in flight), sums them by row with a segmented wave
//           scan and stores one value per row; only rows crossing a chunk boundary use an atomic.
//           A streaming kernel then lands each row sum, tests the threshold and prepares crossing
//           rows for the next level (no atomics on the residue vector; per-workgroup counters go
//           to a partials array that a one-workgroup kernel sums).
//           Forward sweeps of large graphs walk a row-panel or a sliced copy of the in-CSR instead
//           (k_dense_edges_panel + k_panel_fold, k_dense_edges<.., true>).
#include "push_device.hpp"

namespace pprhip {

// State of a dense level (GsState): given by the host, or - for a level launched behind another one without a host
// round trip in between - read from the cell the level before it wrote (kGsNone: that level left nothing to sweep).
__device__ __forceinline__ int dense_state(const int* state_in, int state0) { return state_in ? *state_in : state0; }

// k_dense_edges: one wave per chunk of 512 consecutive in-edges, 8 per lane.  A lane reads its 8
// column indices as two 16-byte loads and one byte of row-start flags, gathers the 8 contributions
// and sums them by row; rows that end inside the wave are completed with a segmented wave scan and
// stored, only the (at most two) rows that cross the chunk boundary use an fp64 atomic.  No LDS,
// no workgroup barrier, no special case for hub rows: every wave carries the same 512 gathers.
constexpr int kHotMax = 16384;  // contributions of the 16K highest-out-degree vertices live in LDS (128 KB)

// The internal vertex order puts the highest out-degrees first (graph lift), so ids < n_hot are the
// contributions gathered most often (42 % of all in-edges at R-MAT scale 22).  A persistent workgroup
// per CU stages them in LDS once per level and serves those gathers from LDS; from L2 every 8-byte
// value costs the L1 a 128-byte line fill, and that line path is what bounds this kernel otherwise
// (250 G gathers/s when everything hits L2; the LDS table buys 19 %).
struct ChunkRegs {  // one lane's share of a chunk: 8 column indices + their row-start flags
  int4 ia, ib;
  uint32_t fb;
};

__device__ __forceinline__ ChunkRegs load_chunk(const int32_t* __restrict__ in_ci,
                                                const uint8_t* __restrict__ start_flags, uint32_t c, int lane) {
  const unsigned long long e0 = (unsigned long long)c * kChunkEdges + 8ull * lane;
  // read once per sweep: non-temporal, so that the index stream does not push gathered lines out of L2
  typedef int v4i __attribute__((ext_vector_type(4)));
  const v4i* q = reinterpret_cast<const v4i*>(in_ci + e0);
  const v4i x = __builtin_nontemporal_load(q), y = __builtin_nontemporal_load(q + 1);
  ChunkRegs r;
  r.ia = make_int4(x.x, x.y, x.z, x.w);
  r.ib = make_int4(y.x, y.y, y.z, y.w);
  r.fb = __builtin_nontemporal_load(&start_flags[e0 >> 3]);
  return r;
}

// Window of a chunk in the launch's virtual order (engine.hpp: EdgeWindows); w only moves forward.
__device__ __forceinline__ uint32_t window_chunk(const EdgeWindows& W, uint32_t vc, uint32_t* w) {
  uint32_t x = *w;
  while (x + 1 < W.n && vc >= W.c_pre[x + 1]) ++x;
  *w = x;
  return W.c_lo[x] + (vc - W.c_pre[x]);
}

// SLICED: the edge arrays are the sliced copy (engine.hpp: SlicedLayout): a flag starts a *segment*, seg_row maps it
// to its row ordinal, and every segment sum is added to the row's accumulator with an fp64 atomic (a row has one
// segment per slice; k_dense_apply leaves the accumulators zero).  Otherwise segments are rows and a row that starts
// and ends inside a chunk is stored.
template <bool HOT, bool SLICED>
__global__ __launch_bounds__(1024) void k_dense_edges(const int32_t* __restrict__ in_ci,
                                                       const uint8_t* __restrict__ start_flags,
                                                       const uint32_t* __restrict__ chunk_starts,
                                                       const uint32_t* __restrict__ seg_row, EdgeWindows W,
                                                       const double* __restrict__ c_cur,
                                                       double* __restrict__ acc_nz, uint32_t n_hot,
                                                       const int* state_in) {
  // One block of a sweep: the chunks that hold the in-edges of the block's rows (the whole CSR when the sweep is not
  // cut into blocks), as a list of windows.  Edges of a boundary chunk outside the window count as zero: the launch
  // (or window) they belong to sums them.
  extern __shared__ __attribute__((aligned(16))) double s_hot[];
  if (dense_state(state_in, kGsJacobi) == kGsNone) return;
  const int lane = lane_id();
  const uint32_t waves_per_block = blockDim.x >> 6;
  const uint32_t stride = gridDim.x * waves_per_block;
  const uint32_t total = W.c_pre[W.n];
  uint32_t vc = blockIdx.x * waves_per_block + (uint32_t)__builtin_amdgcn_readfirstlane(wave_id());
  uint32_t w = 0, c = 0;
  ChunkRegs cur;
  if (vc < total) {
    c = window_chunk(W, vc, &w);
    cur = load_chunk(in_ci, start_flags, c, lane);  // in flight while the hot table loads
  }
  if (HOT) {
    // 16 values per thread, loaded in one batch
    double t[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t i = threadIdx.x + j * 1024u;
      t[j] = i < n_hot ? c_cur[i] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t i = threadIdx.x + j * 1024u;
      if (i < n_hot) s_hot[i] = t[j];
    }
    __syncthreads();
  }
  for (; vc < total; vc += stride) {
    // next chunk's indices are requested before this chunk's gathers, so their latency is hidden
    ChunkRegs nxt = cur;
    uint32_t wn = w, cn = c;
    if (vc + stride < total) {
      cn = window_chunk(W, vc + stride, &wn);
      nxt = load_chunk(in_ci, start_flags, cn, lane);
    }
    const unsigned long long e_lo = W.e_lo[w], e_hi = W.e_hi[w];
    const uint32_t cs = chunk_starts[c];
    const unsigned long long e0 = (unsigned long long)c * kChunkEdges + 8ull * lane;
    const uint32_t fb = cur.fb;
    const int32_t idx[8] = {cur.ia.x, cur.ia.y, cur.ia.z, cur.ia.w, cur.ib.x, cur.ib.y, cur.ib.z, cur.ib.w};
    double v[8];
    if (HOT) {
      // branch-free: every lane issues both loads (hot lanes read c_cur[0], one shared line; cold
      // lanes read s_hot[0]) so that all 8 global gathers of the lane stay in flight together
      double gl[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) gl[i] = c_cur[(uint32_t)idx[i] < n_hot ? 0 : idx[i]];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const double hv = s_hot[(uint32_t)idx[i] < n_hot ? idx[i] : 0];
        v[i] = (uint32_t)idx[i] < n_hot ? hv : gl[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = c_cur[idx[i]];
    }
    if (e0 < e_lo || e0 + 8 > e_hi) {  // first / last chunk of the block only
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (e0 + i < e_lo || e0 + i >= e_hi) v[i] = 0.0;
    }
    // row index of a segment = (row starts at or before its first edge) - 1
    const uint32_t pc = __popc(fb);
    const uint32_t incl = wave_incl_scan_u32_dpp(pc);
    const uint32_t before = cs + incl - pc;  // row starts before this lane's first edge
    double seg = 0.0, first_seg = 0.0;
    uint32_t k = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if ((fb >> i) & 1u) {
        if (k == 0) {
          first_seg = seg;  // closes the row carried in from earlier lanes
        } else if (SLICED) {
          if (seg != 0.0) atomic_add_noret(&acc_nz[seg_row[before + k - 1]], seg);
        } else {
          acc_nz[before + k - 1] = seg;  // a row that starts and ends inside this lane
        }
        seg = 0.0;
        ++k;
      }
      seg += v[i];
    }
    // segmented scan over lanes: S(l) = x(l) + (lane l holds a row start ? 0 : S(l-1))
    const bool h = k != 0;
    const double sval = wave_seg_scan_f64_dpp(seg, h);
    const double carry = wave_prev_f64_dpp(sval);
    const unsigned long long hmask = __ballot(h);
    if (h) {
      // the row that ends at this lane's first start flag: edges carried in + this lane's head
      const bool nonempty = lane > 0 || (fb & 1u) == 0;
      if (nonempty && before > 0) {
        const double tot = carry + first_seg;
        const bool started_here = (hmask & ((1ull << lane) - 1ull)) != 0;  // an earlier lane starts a row
        if (SLICED) {
          if (tot != 0.0) atomic_add_noret(&acc_nz[seg_row[before - 1]], tot);
        } else if (started_here) {
          acc_nz[before - 1] = tot;
        } else {
          atomic_add_noret(&acc_nz[before - 1], tot);  // began in an earlier chunk
        }
      }
    }
    if (lane == 63) {  // the row still open at the end of the chunk
      const uint32_t starts = cs + incl;
      if (starts > 0 && sval != 0.0) atomic_add_noret(&acc_nz[SLICED ? seg_row[starts - 1] : starts - 1], sval);
    }
    cur = nxt;
    w = wn;
    c = cn;
  }
}

// ------------------------------------------------------------------------------------------------
// k_dense_edges_panel (round 6): the single-query forward edge kernel over the row-panel copy (engine_internal.hpp:
// HostPanelLayout).  A workgroup takes an ITEM - at most kItemEdges edges of one panel of kPanelRows rows, sorted by
// source - and sums it into acc[row] in LDS (kPanelLdsBytes, 64 KB).  A wave takes 512 consecutive edges per turn, lane l the edges l,
// l + 64, ... of them (stored as the lane's 32 bytes), the workgroup 8 192: neighbouring lanes gather neighbouring sources, so the sixteen contributions of a 128-byte line are
// one request to the L1 (which keeps ~256 lines in flight per CU - what bounds the row-major and the sliced kernel:
// TCP_PENDING_STALL_CYCLES 0.69 of their cycles), and every workgroup walks the contribution array front to back.  Sums
// land with ds_add_f64 (zero contributions are skipped: a dense level's frontier is a part of the nodes); at the end
// the item's rows leave as one contiguous block part[part0 + row]; k_dense_apply<.., true> adds a row's parts.
// Rows outside [j_lo, j_hi) - the Gauss-Seidel block of the launch, whose bounds may cut a panel - are left out.
// Items are dealt to the workgroups in turn (they are of one size: the parts of a panel hold equal edge counts).
// ------------------------------------------------------------------------------------------------
constexpr int kPanelThreads = 1024;
constexpr int kPanelLdsBytes = (int)(kPanelRows * sizeof(double));
static_assert(kPanelStep == (uint32_t)kPanelThreads * 8u, "eight edges per lane and turn");

__global__ __launch_bounds__(kPanelThreads, 8) void k_dense_edges_panel(const int32_t* __restrict__ src,
                                                                     const uint16_t* __restrict__ rloc,
                                                                     const PanelItem* __restrict__ items,
                                                                     uint32_t item_lo, uint32_t item_hi,
                                                                     const double* __restrict__ c_cur,
                                                                     double* __restrict__ part, uint32_t j_lo,
                                                                     uint32_t j_hi, uint32_t n_nz, const int* state_in,
                                                                     uint32_t* __restrict__ queue) {
  extern __shared__ __attribute__((aligned(16))) double acc[];
  __shared__ uint32_t s_take;
  typedef int v4i __attribute__((ext_vector_type(4)));
  if (dense_state(state_in, kGsJacobi) == kGsNone) return;  // (the queue stays at zero: k_dense_reduce left it so)
  const uint32_t tid = threadIdx.x;
  // items are handed out by a counter (they differ in size by the panels' rounding, and the last round of a static deal
  // would leave most CUs idle); the level's k_dense_reduce zeroes it behind the launch
  uint32_t it = item_lo + blockIdx.x;
  while (it < item_hi) {
    const PanelItem I = items[it];
    if (tid == 0) s_take = atomicAdd(queue, 1u);
    {
      double2* a2 = reinterpret_cast<double2*>(acc);
#pragma unroll
      for (int k = 0; k < (int)(kPanelRows / 2 / kPanelThreads); ++k) a2[(uint32_t)k * kPanelThreads + tid] = make_double2(0.0, 0.0);
    }
    __syncthreads();
    const uint32_t row0 = I.panel * kPanelRows;
    const uint32_t r_lo = j_lo > row0 ? j_lo - row0 : 0u;
    const uint32_t r_hi = j_hi > row0 ? min(min(j_hi, n_nz) - row0, kPanelRows) : 0u;  // (padding: row 0xffff >= r_hi)
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    const v4i* sp = reinterpret_cast<const v4i*>(src + (size_t)I.edge0 * kPanelStep) + 2u * tid;
    const v4u* rp = reinterpret_cast<const v4u*>(rloc + (size_t)I.edge0 * kPanelStep) + tid;
    // the index streams are read once per sweep: non-temporal, so that they do not push gathered lines out of L2
    // (two turns ahead: a turn's index loads are asked for behind the gathers of the turn before the last, so that the
    // wait for a turn's gathers - loads return in order - never waits for the stream from HBM)
    v4i ia = __builtin_nontemporal_load(sp), ib = __builtin_nontemporal_load(sp + 1);
    v4u rx = __builtin_nontemporal_load(rp);
    v4i na = ia, nb = ib;
    v4u nr = rx;
    if (I.steps > 1) {
      na = __builtin_nontemporal_load(sp + (size_t)(2 * kPanelThreads));
      nb = __builtin_nontemporal_load(sp + (size_t)(2 * kPanelThreads) + 1);
      nr = __builtin_nontemporal_load(rp + (size_t)kPanelThreads);
    }
    for (uint32_t i = 0; i < I.steps; ++i) {
      const int32_t u[8] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
      const uint32_t r[8] = {rx.x & 0xffffu, rx.x >> 16, rx.y & 0xffffu, rx.y >> 16,
                             rx.z & 0xffffu, rx.z >> 16, rx.w & 0xffffu, rx.w >> 16};
      bool in[8];
      double v[8];
      // (rows outside the block and the padding gather the first contribution - one shared line - and add nothing)
#pragma unroll
      for (int e = 0; e < 8; ++e) in[e] = r[e] >= r_lo && r[e] < r_hi;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = c_cur[in[e] ? u[e] : 0];
      v4i fa = na, fb = nb;
      v4u fr = nr;
      if (i + 2 < I.steps) {
        fa = __builtin_nontemporal_load(sp + (size_t)(i + 2) * (2 * kPanelThreads));
        fb = __builtin_nontemporal_load(sp + (size_t)(i + 2) * (2 * kPanelThreads) + 1);
        fr = __builtin_nontemporal_load(rp + (size_t)(i + 2) * kPanelThreads);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (in[e] && v[e] != 0.0) atomic_add_noret(&acc[r[e]], v[e]);
      ia = na;
      ib = nb;
      rx = nr;
      na = fa;
      nb = fb;
      nr = fr;
    }
    __syncthreads();
    const uint32_t taken = s_take;  // (written before the barrier above; the next write comes behind the barrier below)
#pragma unroll 4
    for (uint32_t r = tid; r < kPanelRows; r += kPanelThreads)
      if (r >= r_lo && r < r_hi) part[(size_t)I.part0 + r] = acc[r];
    __syncthreads();  // (the accumulators are read: the next item clears them)
    it = item_lo + gridDim.x + taken;
  }
}

// The hub panels' parts: a panel of S > kFoldMin parts has them added kFoldParts at a time first - workgroup (x, g)
// adds the parts [g kFoldParts, ...) of 256 rows, the loads of a lane independent of one another - so that k_dense_apply
// adds ceil(S / kFoldParts) values per row instead of hundreds in a chain.  Rows outside [j_lo, j_hi) are left alone.
__global__ __launch_bounds__(256) void k_panel_fold(double* __restrict__ part, const PanelDesc* __restrict__ panels,
                                                    uint32_t panel, uint32_t j_lo, uint32_t j_hi, const int* state_in) {
  if (dense_state(state_in, kGsJacobi) == kGsNone) return;
  panel += blockIdx.z;
  const PanelDesc P = panels[panel];
  const uint32_t r = blockIdx.x * 256u + threadIdx.x, g = blockIdx.y, j = panel * kPanelRows + r;
  if (P.fold == kNoFold || r >= P.rows || j < j_lo || j >= j_hi) return;
  const uint32_t k0 = g * kFoldParts, k1 = min(P.parts, k0 + kFoldParts);
  if (k0 >= P.parts) return;
  const double* p = part + (size_t)P.base + r;
  double x[kFoldParts];
#pragma unroll
  for (uint32_t k = 0; k < kFoldParts; ++k) x[k] = k0 + k < k1 ? p[(size_t)(k0 + k) * P.rows] : 0.0;
  double v = 0.0;
#pragma unroll
  for (uint32_t k = 0; k < kFoldParts; ++k) v += x[k];
  part[(size_t)P.fold + (size_t)g * P.rows + r] = v;
}

// k_dense_apply: one thread per non-empty row (plus one for a source without in-edges, which
// only ever receives returned dead-end mass): lands the row sum, detects the threshold crossing
// and prepares the row for the next level in place.
// PANEL: the row sum arrives as the S parts k_dense_edges_panel's items left (acc_nz = their buffer; panels = PanelDesc).
template <int MODE, bool PANEL>
__global__ __launch_bounds__(256) void k_dense_apply(const int32_t* __restrict__ nz_rows, uint32_t j_lo, uint32_t n_nz,
                                                      double* __restrict__ acc_nz, const PanelDesc* __restrict__ panels,
                                                      const uint32_t* __restrict__ out_rp,
                                                      const uint32_t* __restrict__ in_rp,
                                                      double* __restrict__ c_cur, double* __restrict__ c_next,
                                                      double* __restrict__ res,
                                                      double* __restrict__ reserve, uint8_t* __restrict__ flags,
                                                      uint32_t* __restrict__ armed,
                                                      DevCounters* ctr, unsigned long long* __restrict__ blk_pack,
                                                      double* __restrict__ blk_dead, uint32_t* __restrict__ blk_ndead,
                                                      int dead_slot, int src_extra, PushArgs a,
                                                      const int* state_in, int state0, int last_block,
                                                      const double* __restrict__ seed_w,
                                                      const int32_t* __restrict__ extra_rows) {
  // rows [j_lo, n_nz) of one block (n_nz = the block's end; + the source without in-edges behind the last block)
  __shared__ double s_red[4];
  __shared__ unsigned long long s_red2[4];
  const int state = dense_state(state_in, state0);
  if (state == kGsNone) return;
  const int tid = threadIdx.x;
  const uint32_t j = j_lo + blockIdx.x * 256u + tid;
  bool have = false;
  int32_t u = -1;
  double acc = 0.0;
  if (j < n_nz) {
    u = nz_rows[j];
    if (PANEL) {
      const PanelDesc P = panels[j / kPanelRows];  // (a wave's rows lie in one panel or two: uniform loads)
      const bool folded = P.fold != kNoFold;
      const double* p = acc_nz + (size_t)(folded ? P.fold : P.base) + (j % kPanelRows);
      const uint32_t cnt = folded ? (P.parts + kFoldParts - 1) / kFoldParts : P.parts;
      uint32_t k = 0;
      for (; k + 4 <= cnt; k += 4) {
        const double x0 = p[(size_t)k * P.rows], x1 = p[(size_t)(k + 1) * P.rows], x2 = p[(size_t)(k + 2) * P.rows],
                     x3 = p[(size_t)(k + 3) * P.rows];
        acc = (((acc + x0) + x1) + x2) + x3;
      }
      for (; k < cnt; ++k) acc += p[(size_t)k * P.rows];
    } else {
      acc = acc_nz[j];
      acc_nz[j] = 0.0;
    }
    have = true;
  } else if (j - n_nz < (uint32_t)src_extra) {  // (j >= n_nz here)
    u = extra_rows ? extra_rows[j - n_nz] : a.src;
    have = true;
  }
  double dead_next = 0.0;
  unsigned long long pack = 0, ndead = 0;
  if (have) {
    if (MODE != kBackward && u == a.src) {
      const double dd = ctr->dead[dead_slot];
      if (dd > 0.0) {
        acc += dd;
        ctr->dead[dead_slot] = 0.0;
      }
    } else if (MODE != kBackward && seed_w) {
      // seed set: the level's dead-end mass lands on the live seeds as p does (k_seed_land_dense zeroes the cell)
      const double w = seed_w[u];
      if (w != 0.0) {
        const double dd = ctr->dead[dead_slot];
        if (dd > 0.0) acc += dd * w;
      }
    }
    const uint32_t d = out_rp[u + 1] - out_rp[u];
    double cn = 0.0;
    if (MODE == kBackward) {
      // Backward_Search.java:73-96 in pull form over the out-CSR: the row's out-neighbours gave (1 - alpha) *
      // residue each, this row takes its share 1 / d_out; strict un-normalised threshold (:89)
      if (acc > 0.0) {
        const double old = res[u];
        const double nw = old + acc / (double)d;
        if (!(old > a.rmax) && nw > a.rmax) {
          reserve[u] = reserve[u] + nw * a.alpha;
          if (old != 0.0) res[u] = 0.0;
          cn = (1.0 - a.alpha) * nw;
          pack = (1ull << kPackShift) | (unsigned long long)(in_rp[u + 1] - in_rp[u]);
        } else {
          res[u] = nw;
        }
      }
    } else if (acc > 0.0) {
      const double old = res[u];
      const double nw = old + acc;
      bool crossing = (MODE == kPower) ? true : (!active_fwd(old, d, a.rmax) && active_fwd(nw, d, a.rmax));
      if (MODE == kFwdTopk) {
        // a row is applied once per level, so "receives mass and meets the threshold" needs no queue test here: an
        // armed node (met the threshold at round start, not queued) joins with its first mass (:226-231)
        if (a.rmax < a.min_rmax && active_fwd(old, d, a.rmax)) crossing = take_armed(armed, u);
        if (active_fwd(nw, d, a.min_rmax)) flags[u] = 1;
      }
      if (crossing) {  // becomes a frontier node of the next level: prepare it right here
        reserve[u] = reserve[u] + nw * a.alpha;
        if (old != 0.0) res[u] = 0.0;
        if (d == 0) {
          dead_next = nw * (1.0 - a.alpha);
          ndead = 1;
        } else {
          cn = ((1.0 - a.alpha) * nw) / (double)d;
        }
        pack = (1ull << kPackShift) | (unsigned long long)d;
      } else {
        res[u] = nw;
      }
    }
    c_next[u] = cn;
    // what the later blocks of this sweep read from the current array (engine.hpp: GsState); nobody reads the last
    // block's rows again in this sweep, and the next sweep reads c_next
    if (!last_block) {
      if (state == kGsEntry) c_cur[u] = c_cur[u] + cn;
      else if (state == kGsInPlace) c_cur[u] = cn;
      else if (state == kGsFlush) c_cur[u] = 0.0;
    }
  }
  // per-workgroup partials; k_dense_reduce sums them (no same-address atomics in this kernel)
  const double ds = block_sum_f64(dead_next, s_red);
  const unsigned long long ps = block_sum_u64(pack, s_red2);
  const unsigned long long nd = block_sum_u64(ndead, s_red2);
  if (tid == 0) {
    blk_pack[blockIdx.x] = ps;
    blk_dead[blockIdx.x] = ds;
    blk_ndead[blockIdx.x] = (uint32_t)nd;
  }
}

// sums the per-workgroup partials of a dense level into the level counter, the dead-mass cell
// and the dead-end pop count
__global__ __launch_bounds__(1024) void k_dense_reduce(const unsigned long long* __restrict__ blk_pack,
                                                        const double* __restrict__ blk_dead,
                                                        const uint32_t* __restrict__ blk_ndead, uint32_t n_blocks,
                                                        DevCounters* ctr, int out_slot, int dead_slot_next,
                                                        const int* state_in, int state0, unsigned long long* hist_out,
                                                        int* state_out, unsigned long long dense_thresh,
                                                        unsigned long long gs_thresh, uint32_t* queues) {
  __shared__ double s_red[16];
  __shared__ unsigned long long s_red2[16];
  if (queues && threadIdx.x < kPanelQueues) queues[threadIdx.x] = 0u;  // the item queues of this level's panel launches
  const int state = dense_state(state_in, state0);
  if (state == kGsNone) {
    if (threadIdx.x == 0 && state_out) *state_out = kGsNone;
    return;
  }
  unsigned long long pack = 0, ndead = 0;
  double dead = 0.0;
  for (uint32_t i = threadIdx.x; i < n_blocks; i += blockDim.x) {
    pack += blk_pack[i];
    if (blk_dead) {
      dead += blk_dead[i];
      ndead += blk_ndead[i];
    }
  }
  const unsigned long long ps = block_sum_u64(pack, s_red2);
  const unsigned long long nd = block_sum_u64(ndead, s_red2);
  const double ds = block_sum_f64(dead, s_red);
  if (threadIdx.x == 0) {
    ctr->packed[out_slot] = ps;
    if (hist_out) *hist_out = ps;
    if (state_out) *state_out = gs_next_state(state, ps >> kPackShift, ps & kPackMask, dense_thresh, gs_thresh);
    if (nd) {
      ctr->dead[dead_slot_next] = ctr->dead[dead_slot_next] + ds;
      ctr->dead_pops += nd;
    }
  }
}

// After a dense level's apply kernels: the live seeds took their share x q_i inside the apply (seed_w), like the source
// row of a single-source query; here the dead-end seeds take x e_j and the cell is cleared.
__global__ __launch_bounds__(256) void k_seed_land_dense(const int32_t* __restrict__ id, const double* __restrict__ w,
                                                          uint32_t n_live, uint32_t n_all, unsigned int* done,
                                                          double* __restrict__ reserve, DevCounters* ctr, int dead_slot,
                                                          const int* state_in, int state0) {
  if (dense_state(state_in, state0) == kGsNone) return;
  const double x = ctr->dead[dead_slot];
  if (!(x > 0.0)) return;
  for (uint32_t i = n_live + blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += gridDim.x * blockDim.x)
    reserve[id[i]] = reserve[id[i]] + x * w[i];
  seed_land_done(done, ctr, dead_slot);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
int launch_dense_level(pprhip_graph* g, const PushArgs& a, int cbuf, int out_slot, int dead_slot,
                       const DenseLaunch& dl) {
  // (the layout of the side the level sweeps was built by the caller)
  const bool bwd = a.mode == kBackward;
  SweepSide side = sweep_side(g->gr, bwd);
  const uint32_t n_nz = side.n_nz;
  // a source without in-edges still receives returned dead-end mass: one extra apply thread, behind the last block
  // (a seed set: one per live seed without in-edges; the live seeds' landing weights go to the apply kernel)
  const SeedTable* sd = (!bwd && g->seed_on) ? g->seeds : nullptr;
  const int src_extra = sd ? (int)sd->n_zin : (!bwd && a.src >= 0 && g->gr->h_in_rp[a.src + 1] == g->gr->h_in_rp[a.src]) ? 1 : 0;
  const double* seed_w = sd ? sd->w_node : nullptr;
  const int32_t* extra_rows = sd ? sd->zin : nullptr;
  const GsBlock whole{0u, n_nz, 0ull, (unsigned long long)g->gr->m};
  const GsBlock* blocks = (dl.blocks && dl.n_blocks > 1 && !bwd) ? dl.blocks : &whole;
  const int nb = blocks == &whole ? 1 : dl.n_blocks;
  const uint32_t n_hot = g->gr->relabeled ? std::min<uint32_t>(g->gr->n, (uint32_t)kHotMax) : 0u;
  // forward sweeps walk the row-panel copy of the in-CSR where the graph has one (from 2^26 edges on) and the handle
  // has the buffer of its parts' sums (ensure_panel_part), else - a graph whose sources span several slices - the sliced
  // copy
  const PanelLayout* pn = (!bwd && g->gr->pn && g->pn_part) ? g->gr->pn : nullptr;
  const SlicedLayout* sl = (bwd || pn) ? nullptr : g->gr->sl;
  const EdgeWindows* wins = sl ? detail::sliced_windows_of(g, blocks == &whole ? nullptr : blocks, nb) : nullptr;
  if (sl) {  // (its edge arrays in place of the in-CSR's)
    side.ci = sl->ci;
    side.start_flags = sl->flags;
    side.chunk_starts = sl->chunk_starts;
  }
  // the apply kernel of the level: its row sums are the panel items' parts, or lie in acc_nz
  decltype(&k_dense_apply<kPower, false>) apply = nullptr;
  DISPATCH_MODE(a.mode, apply = pn ? &k_dense_apply<M, true> : &k_dense_apply<M, false>);
  uint32_t part_base = 0;
  for (int b = 0; b < nb; ++b) {
    const GsBlock& B = blocks[b];
    EdgeWindows one;
    if (!sl) {
      one.n = 1;
      one.c_pre[0] = 0;
      one.c_lo[0] = (uint32_t)(B.e_lo / kChunkEdges);
      one.c_pre[1] = (uint32_t)((B.e_hi + kChunkEdges - 1) / kChunkEdges) - one.c_lo[0];
      one.e_lo[0] = B.e_lo;
      one.e_hi[0] = B.e_hi;
    }
    const EdgeWindows& W = sl ? wins[b] : one;
    const uint32_t n_ch = W.n ? W.c_pre[W.n] : 0u;
    if (pn) {
      // block boundaries are multiples of 256 row ordinals and may cut a panel: the kernel leaves the other rows out
      const uint32_t p_lo = B.j_lo / kPanelRows, p_hi = std::min<uint32_t>(pn->n_panels, (B.j_hi + kPanelRows - 1) / kPanelRows);
      const uint32_t i_lo = p_hi > p_lo ? pn->h_panel_item0[p_lo] : 0u, i_hi = p_hi > p_lo ? pn->h_panel_item0[p_hi] : 0u;
      if (i_hi > i_lo) {
        const uint32_t grid = std::min<uint32_t>(i_hi - i_lo, (uint32_t)g->gr->n_cus * (uint32_t)(160 * 1024 / (kPanelLdsBytes + 1024)));
        k_dense_edges_panel<<<dim3(grid), dim3(kPanelThreads), kPanelLdsBytes, g->stream>>>(
            pn->src, pn->rloc, pn->items, i_lo, i_hi, g->cdense[cbuf], g->pn_part, B.j_lo, B.j_hi, n_nz, dl.state_in,
            g->pn_ctr + std::min(b, kPanelQueues - 1));
        PPRHIP_CHECK_HIP(hipGetLastError());
        // panels of many parts (the hub rows': the first few - rows are ordered by degree, so parts do not grow)
        uint32_t p_fold = p_lo, s_max = 0;
        for (uint32_t p = p_lo; p < p_hi; ++p) {
          const uint32_t S = pn->h_panel_item0[p + 1] - pn->h_panel_item0[p];
          if (S > kFoldMin) {
            p_fold = p + 1;
            s_max = std::max(s_max, S);
          }
        }
        if (p_fold > p_lo) {
          k_panel_fold<<<dim3(kPanelRows / 256, (s_max + kFoldParts - 1) / kFoldParts, p_fold - p_lo), dim3(256), 0, g->stream>>>(
              g->pn_part, pn->panels, p_lo, B.j_lo, B.j_hi, dl.state_in);
          PPRHIP_CHECK_HIP(hipGetLastError());
        }
      }
    } else if (g->gr->n_chunks && n_ch) {
      // persistent workgroups: one 1024-thread workgroup per CU when the LDS hot table is in use
      const uint32_t want = (n_ch + 15) / 16;
      const uint32_t grid = std::min<uint32_t>(want, (uint32_t)g->gr->n_cus * (n_hot ? 1u : 2u));
      const size_t lds = n_hot ? sizeof(double) * n_hot : 0;  // (above 64 KB: opted in by init_kernels_dense)
      if (n_hot && sl)
        k_dense_edges<true, true><<<dim3(grid), dim3(1024), lds, g->stream>>>(
            side.ci, side.start_flags, side.chunk_starts, sl->seg_row, W, g->cdense[cbuf], g->acc_nz, n_hot, dl.state_in);
      else if (n_hot)
        k_dense_edges<true, false><<<dim3(grid), dim3(1024), lds, g->stream>>>(
            side.ci, side.start_flags, side.chunk_starts, nullptr, W, g->cdense[cbuf], g->acc_nz, n_hot, dl.state_in);
      else if (sl)
        k_dense_edges<false, true><<<dim3(grid), dim3(1024), 0, g->stream>>>(
            side.ci, side.start_flags, side.chunk_starts, sl->seg_row, W, g->cdense[cbuf], g->acc_nz, 0u, dl.state_in);
      else
        k_dense_edges<false, false><<<dim3(grid), dim3(1024), 0, g->stream>>>(
            side.ci, side.start_flags, side.chunk_starts, nullptr, W, g->cdense[cbuf], g->acc_nz, 0u, dl.state_in);
      PPRHIP_CHECK_HIP(hipGetLastError());
    }
    const int extra = (b == nb - 1) ? src_extra : 0;
    const uint32_t rows = B.j_hi - B.j_lo + (uint32_t)extra;
    const uint32_t grid = (rows + 255) / 256;
    if (grid) {
      apply<<<dim3(grid), dim3(256), 0, g->stream>>>(
          side.nz_rows, B.j_lo, B.j_hi, pn ? g->pn_part : g->acc_nz, pn ? pn->panels : nullptr, g->gr->out_rp, g->gr->in_rp,
          g->cdense[cbuf], g->cdense[cbuf ^ 1], g->residue, g->reserve, g->flags, g->armed, g->ctr, g->blk_pack + part_base,
          g->blk_dead + part_base, g->blk_ndead + part_base, dead_slot, extra, a, dl.state_in, dl.state0,
          b == nb - 1 ? 1 : 0, seed_w, extra_rows);
      PPRHIP_CHECK_HIP(hipGetLastError());
      part_base += grid;
    }
  }
  if (sd) {
    k_seed_land_dense<<<dim3(grid_for(sd->n_dead, 256, 1024)), dim3(256), 0, g->stream>>>(
        sd->id, sd->w, sd->n_live, sd->n_live + sd->n_dead, sd->done, g->reserve, g->ctr, dead_slot, dl.state_in, dl.state0);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  k_dense_reduce<<<dim3(1), dim3(1024), 0, g->stream>>>(g->blk_pack, g->blk_dead, g->blk_ndead, part_base, g->ctr,
                                                        out_slot, dead_slot ^ 1, dl.state_in, dl.state0, dl.hist_out,
                                                        dl.state_out, dl.dense_thresh, dl.gs_thresh, pn ? g->pn_ctr : nullptr);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int reduce_partials(pprhip_graph* g, uint32_t n_blocks, int out_slot, int dead_slot, bool with_dead) {
  k_dense_reduce<<<dim3(1), dim3(1024), 0, g->stream>>>(g->blk_pack, with_dead ? g->blk_dead : nullptr, g->blk_ndead,
                                                        n_blocks, g->ctr, out_slot, dead_slot, nullptr, kGsJacobi, nullptr,
                                                        nullptr, 0ull, ~0ull, nullptr);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// Current device: code object loaded, large dynamic LDS opted in (above 64 KB it needs an explicit opt-in per
// device; see init_kernels_push).
int init_kernels_dense() {
  PPRHIP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dense_edges<true, false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * kHotMax)));
  PPRHIP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dense_edges<true, true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * kHotMax)));
  PPRHIP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dense_edges_panel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kPanelLdsBytes));
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_dense_reduce)));
  return PPRHIP_OK;
}

}  // namespace pprhip
