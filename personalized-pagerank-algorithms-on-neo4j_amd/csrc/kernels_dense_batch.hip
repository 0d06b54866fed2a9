// kernels_dense_batch.hip — the dense level of sixteen queries at once (the batched sweep) for gfx950 (MI355X).
//
// A gather moves a 128-byte line whether 8 bytes of it are used or all of it, and the rate of lines
// that leave L2 (52-55 G/s = the HBM roof at line granularity) is what bounds the sweep: the edge
// kernel below runs at 51.7 G lines/s.  The batched sweep keeps the contributions of
// kBatch = 16 concurrent queries interleaved, c8[v][slot] (128 bytes per vertex = one L2 line), so
// the line a gather brings in carries that vertex's contribution for every query in flight, and
// the column indices are read once for all of them.  G = kBatch lanes (one per slot) share an
// edge: a wave still owns a 512-edge chunk, lane group g = lane / G walks edges [8Gg, 8G(g+1)) of
// it in order.  The group's column indices sit in its own lanes' registers (two coalesced 16-byte
// loads per lane) and are broadcast inside the group with ds_swizzle; row sums close inside the
// group where a row starts and ends there, cross groups with a short segmented scan, and only rows
// crossing the chunk boundary use atomics.  (Measured on R-MAT 22, all slots busy: 0.69 ms per
// sweep at G = 8, 0.83 ms at G = 16, 1.85 ms at G = 32.)
#include "push_device.hpp"

namespace pprhip {

constexpr int kHotBytes = 128 * 1024;  // LDS table of the hottest vertices' lines (2048 x 64 B or 1024 x 128 B)
// The batched edge kernel takes 32 KB of it (256 lines) since round 5: the table's size never mattered to the sweep
// itself (0 / 256 / 512 / 1024 lines within 0.5 %, round 2), but a workgroup that holds 128 of a CU's 160 KB keeps
// every kernel with a larger LDS block of its own - the sparse push's 48 KB - off the CU while it runs, and the
// queries that work beside the sweeps (batch_driver.hpp: SlotDriver) wait for the gaps between the sweep's kernels:
// k_sparse_push took 99 us per launch beside the sweeps against 14 us alone.  128 -> 32 KB: 344-347 -> 352 queries/s.
constexpr int kHotDefaultBytes = 32 * 1024;

// value of lane K of the caller's lane group (G = 8 or 16 lanes)
template <int G, int K>
__device__ __forceinline__ int group_bcast(int x) {
  return __builtin_amdgcn_ds_swizzle(x, (0x1f & ~(G - 1)) | (K << 5));
}

template <int G>
struct ChunkRegsB {
  int4 ia, ib;
  unsigned long long mask[G / 8];  // row-start bits of the lane group's 8 * G edges
};

template <int G>
__device__ __forceinline__ ChunkRegsB<G> load_chunk_b(const int32_t* __restrict__ in_ci,
                                                      const unsigned long long* __restrict__ flags64, uint32_t c,
                                                      int lane) {
  const unsigned long long e0 = (unsigned long long)c * kChunkEdges + 8ull * lane;
  const int4* p = reinterpret_cast<const int4*>(in_ci + e0);
  ChunkRegsB<G> r;
  // the index stream is read once per sweep: non-temporal, so that it does not push gathered lines out of L2
  typedef int v4i __attribute__((ext_vector_type(4)));
  const v4i* q = reinterpret_cast<const v4i*>(p);
  const v4i x = __builtin_nontemporal_load(q), y = __builtin_nontemporal_load(q + 1);
  r.ia = make_int4(x.x, x.y, x.z, x.w);
  r.ib = make_int4(y.x, y.y, y.z, y.w);
#pragma unroll
  for (int w = 0; w < G / 8; ++w)
    r.mask[w] = __builtin_nontemporal_load(&flags64[(size_t)c * 8 + (size_t)(lane / G) * (G / 8) + w]);
  return r;
}

// 8 edges of the group: the indices sit in lane JB of the group.
template <bool HOT, int G, int JB>
__device__ __forceinline__ void edges_b_block(const ChunkRegsB<G>& cur, const double* __restrict__ cB,
                                              const double* s_hot, uint32_t n_hot, int s, bool tail,
                                              unsigned long long e_first, unsigned long long e_lo,
                                              unsigned long long e_hi, uint32_t before,
                                              double* __restrict__ accB, double& seg, double& first_seg, uint32_t& k) {
  const int32_t own[8] = {cur.ia.x, cur.ia.y, cur.ia.z, cur.ia.w, cur.ib.x, cur.ib.y, cur.ib.z, cur.ib.w};
  uint32_t v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (uint32_t)group_bcast<G, JB>(own[i]);
  double val[8];
  if (HOT) {
    double gl[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) gl[i] = cB[(size_t)(v[i] < n_hot ? 0u : v[i]) * G + s];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double hv = s_hot[(v[i] < n_hot ? v[i] : 0u) * G + s];
      val[i] = v[i] < n_hot ? hv : gl[i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) val[i] = cB[(size_t)v[i] * G + s];
  }
  if (tail) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (e_first + JB * 8 + i < e_lo || e_first + JB * 8 + i >= e_hi) val[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if ((cur.mask[(JB * 8 + i) >> 6] >> ((JB * 8 + i) & 63)) & 1ull) {
      if (k == 0)
        first_seg = seg;  // closes the row carried in from earlier groups
      else
        __builtin_nontemporal_store(seg, &accB[(size_t)(before + k - 1) * G + s]);  // a row that starts and ends inside this group
      seg = 0.0;
      ++k;
    }
    seg += val[i];
  }
}

template <bool HOT, int G, int JB>
struct EdgeBlocks {
  static __device__ __forceinline__ void run(const ChunkRegsB<G>& cur, const double* __restrict__ cB,
                                             const double* s_hot, uint32_t n_hot, int s, bool tail,
                                             unsigned long long e_first, unsigned long long e_lo,
                                             unsigned long long e_hi, uint32_t before,
                                             double* __restrict__ accB, double& seg, double& first_seg, uint32_t& k) {
    EdgeBlocks<HOT, G, JB - 1>::run(cur, cB, s_hot, n_hot, s, tail, e_first, e_lo, e_hi, before, accB, seg, first_seg, k);
    edges_b_block<HOT, G, JB>(cur, cB, s_hot, n_hot, s, tail, e_first, e_lo, e_hi, before, accB, seg, first_seg, k);
  }
};
template <bool HOT, int G>
struct EdgeBlocks<HOT, G, -1> {
  static __device__ __forceinline__ void run(const ChunkRegsB<G>&, const double*, const double*, uint32_t, int, bool,
                                             unsigned long long, unsigned long long, unsigned long long, uint32_t,
                                             double*, double&, double&, uint32_t&) {}
};

// G = queries per sweep = lanes per edge; the wave's 64 / G lane groups walk 8 * G edges each.
template <bool HOT, int G>
__global__ __launch_bounds__(1024) void k_dense_edges_b(const int32_t* __restrict__ in_ci,
                                                         const unsigned long long* __restrict__ flags64,
                                                         const uint32_t* __restrict__ chunk_starts, uint32_t n_chunks,
                                                         unsigned long long m, const double* __restrict__ cB,
                                                         double* __restrict__ accB, uint32_t n_hot, uint32_t c_lo,
                                                         unsigned long long e_lo, unsigned long long e_hi, uint32_t n) {
  // one block of a sweep: chunks [c_lo, n_chunks) holding the in-edges [e_lo, e_hi) (see k_dense_edges)
  extern __shared__ __attribute__((aligned(16))) double s_hot[];
  const int lane = lane_id();
  const int grp = lane / G, s = lane & (G - 1);
  const uint32_t waves_per_block = blockDim.x >> 6;
  const uint32_t stride = gridDim.x * waves_per_block;
  uint32_t c = c_lo + blockIdx.x * waves_per_block + (uint32_t)wave_id();
  ChunkRegsB<G> cur;
  if (c < n_chunks) cur = load_chunk_b<G>(in_ci, flags64, c, lane);
  if (HOT) {
    double t[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t i = threadIdx.x + j * 1024u;
      t[j] = i < n_hot * G ? cB[i] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t i = threadIdx.x + j * 1024u;
      if (i < n_hot * G) s_hot[i] = t[j];
    }
    __syncthreads();
  }
  for (; c < n_chunks; c += stride) {
    ChunkRegsB<G> nxt = cur;
    const uint32_t cn = c + stride;
    if (cn < n_chunks) nxt = load_chunk_b<G>(in_ci, flags64, cn, lane);
    const uint32_t cs = chunk_starts[c];
    uint32_t pc = 0;
#pragma unroll
    for (int w = 0; w < G / 8; ++w) pc += (uint32_t)__popcll(cur.mask[w]);
    const uint32_t incl = wave_incl_scan_u32_dpp(s == 0 ? pc : 0u);  // row starts up to and including this group
    const uint32_t before = cs + incl - pc;
    const unsigned long long e_first = (unsigned long long)c * kChunkEdges + (unsigned long long)(8 * G) * grp;
    const unsigned long long c_e0 = (unsigned long long)c * kChunkEdges;
    const bool tail = c_e0 < e_lo || c_e0 + kChunkEdges > e_hi;  // first / last chunk of the block: edges outside count 0
    double seg = 0.0, first_seg = 0.0;
    uint32_t k = 0;
    EdgeBlocks<HOT, G, G - 1>::run(cur, cB, s_hot, n_hot, s, tail, e_first, e_lo, e_hi, before, accB, seg, first_seg, k);
    // segmented scan over the lane groups: S(g) = tail(g) + (group g holds a row start ? 0 : S(g-1))
    const bool h = k != 0;
    double S = seg;
    int F = h ? 1 : 0;
#pragma unroll
    for (int d = G; d < 64; d <<= 1) {
      const double ps = __shfl_up(S, d);
      const int pf = __shfl_up(F, d);
      if (lane >= d) {
        if (!F) S += ps;
        F |= pf;
      }
    }
    double carry = __shfl_up(S, G);
    if (lane < G) carry = 0.0;
    const unsigned long long hmask = __ballot(h);
    if (h) {
      const bool nonempty = grp > 0 || (cur.mask[0] & 1ull) == 0;
      if (nonempty && before > 0) {
        const double total = carry + first_seg;
        const bool started_here = (hmask & ((1ull << (grp * G)) - 1ull)) != 0;
        double* dst = &accB[(size_t)(before - 1) * G + s];
        if (started_here)
          *dst = total;
        else
          atomic_add_noret(dst, total);  // began in an earlier chunk
      }
    }
    if (grp == 64 / G - 1) {  // the row still open at the end of the chunk
      const uint32_t starts = cs + incl;
      if (starts > 0 && S != 0.0) atomic_add_noret(&accB[(size_t)(starts - 1) * G + s], S);
    }
    cur = nxt;
  }
}

// k_dense_apply_batch: the batched form of k_dense_apply.  Rows without in-edges that can be a query's source
// (those with out-edges) are included: their contribution for the next level is written as 0, or holds the source's
// returned dead-end mass.  So the sweep rewrites every entry of c8_next that can ever be non-zero (isolated nodes'
// entries are never written and stay zero) and a column a slot has left stays all-zero.
// A workgroup takes 64 rows at a time through an LDS tile [row][slot]: row sums come in and next
// contributions go out in the interleaved layout (whole 128-byte lines), while the per-slot
// residue / reserve vectors are walked with a lane per row, i.e. coalesced as in the single-query
// kernel.  Wave w serves kSlotsPerWave consecutive slots; slot arguments are
// wave-uniform.  Counters go to per-slot partials.
constexpr int kApplyRows = 64;
constexpr int kApplyGroups = 2;  // tiles of kApplyRows rows a workgroup carries through its phases together
constexpr int kApplyThreads = 512;  // 8 waves, 2 slots each: few enough slot arguments to stay in SGPRs
constexpr int kSlotsPerWave = kBatch / (kApplyThreads / 64);
// flags of a launch: the tiles' classes count; (hooks library) the residues of dead-end tiles are loaded and counted;
// dead-end tiles are staged and stored as plain ones are (their residues still count as zero)
constexpr uint32_t kApplyLean = 1u;
#ifdef PPRHIP_TEST_HOOKS
constexpr uint32_t kApplyCountRes = 2u;
#endif
constexpr uint32_t kApplyStoreDead = 4u;
// a dead-end tile of a launch with kApplyStoreDead, inside the kernel only (bit 0: the rows are dead ends)
constexpr uint32_t kTileDeadEndStored = 3u;
static_assert((kTileDeadEnd & 1u) && !(kTilePlain & 1u) && !(kTileNoIn & 1u), "bit 0 of a class says dead end");

// The slot vectors' pointers come out of SlotArgs in memory, so the compiler takes them for generic pointers and uses
// flat_* instructions, which also count on lgkmcnt; they are device memory.
template <class T>
__device__ __forceinline__ T __attribute__((address_space(1)))* slot_vec(T* p) {
  return (T __attribute__((address_space(1)))*)p;
}
// take_armed (push_device.hpp) on a slot's armed bits
__device__ __forceinline__ bool take_armed_slot(uint32_t* armed_generic, int32_t u) {
  auto armed = slot_vec(armed_generic);
  const uint32_t bit = 1u << ((uint32_t)u & 31u);
  if (!(armed[(uint32_t)u >> 5] & bit)) return false;
  return (__hip_atomic_fetch_and(&armed[(uint32_t)u >> 5], ~bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) != 0;
}

constexpr int kApplyPerThread = kApplyRows * kBatch / kApplyThreads;  // row sums of a tile a thread moves

// What a trip needs from memory before its first barrier, loaded in one flight: no load below depends on another or
// stands behind a branch (a row behind the last with edges reads row 0's sums, a tile behind tile_hi what is there,
// and the trip counts both as 0.0; the records behind the last row hold node -1), so a trip waits for memory once
// where it used to wait for every row sum and then for nz_rows -> out_rp.
struct ApplyFlight {
  double v[kApplyGroups][kApplyPerThread];  // row sums, as the tile's [row][slot] lines (out of range: row 0's)
  uint4 md;                                 // threads below kApplyRows * kApplyGroups: the record of row tid of the trip
  unsigned long long cw[kApplyGroups];      // cross bits of the tiles
};
__device__ __forceinline__ void apply_flight(ApplyFlight& f, uint32_t tl0, uint32_t n_nz, const double* acc8,
                                             const uint4* __restrict__ meta,
                                             const unsigned long long* __restrict__ cross_bits, int tid) {
  if (tid < kApplyRows * kApplyGroups) f.md = meta[(size_t)tl0 * kApplyRows + tid];  // (whole waves take the branch)
#pragma unroll
  for (int g = 0; g < kApplyGroups; ++g) {
    const uint32_t tl = tl0 + g;  // (at most the tile behind the last: cross_bits has a word for it)
    f.cw[g] = cross_bits[tl];
#pragma unroll
    for (int i = 0; i < kApplyPerThread; ++i) {
      const uint32_t idx = (uint32_t)i * (uint32_t)kApplyThreads + tid;
      const uint32_t j = tl * kApplyRows + idx / kBatch;
      f.v[g][i] = __builtin_nontemporal_load(&acc8[(size_t)(j < n_nz ? j : 0u) * kBatch + idx % kBatch]);
    }
  }
}

// records of the apply kernel's rows on one sweep side (BatchState::apply_meta), n_pad of them
__global__ __launch_bounds__(256) void k_build_apply_meta(const int32_t* __restrict__ nz_rows, uint32_t n_nz,
                                                          const int32_t* __restrict__ z_rows, uint32_t n_z,
                                                          const uint32_t* __restrict__ out_rp,
                                                          const uint32_t* __restrict__ in_rp_bwd, uint4* __restrict__ meta,
                                                          uint32_t n_pad) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n_pad) return;  // (n_pad is a multiple of 128: whole waves, i.e. whole tiles, return)
  const int32_t u = j < n_nz ? nz_rows[j] : (j < n_nz + n_z ? z_rows[j - n_nz] : -1);
  uint4 r = make_uint4((uint32_t)u, 0u, 0u, 0u);
  if (u >= 0) {
    r.y = out_rp[u + 1] - out_rp[u];
    if (in_rp_bwd) r.z = in_rp_bwd[u + 1] - in_rp_bwd[u];
  }
  // the tile's class (engine.hpp: ApplyTileClass), from the records themselves: a wave holds one tile
  if (!in_rp_bwd) {
    const bool dead_end = u >= 0 && j < n_nz && r.y == 0u;
    if (__ballot(dead_end) == ~0ull) r.w = kTileDeadEnd;
    if (__ballot(j >= n_nz) == ~0ull) r.w = kTileNoIn;
  }
  meta[j] = r;
}

__global__ __launch_bounds__(kApplyThreads) void k_dense_apply_batch(const uint4* __restrict__ meta, uint32_t n_nz,
                                                            uint32_t n_zin, double* __restrict__ acc8,
                                                            double* __restrict__ c8_cur, double* __restrict__ c8_next,
                                                            uint32_t tile_lo, uint32_t tile_hi, uint32_t gs_mask,
                                                            uint32_t entry_mask,
                                                            const SlotArgs* __restrict__ slots,
                                                            const unsigned long long* __restrict__ cross_bits,
                                                            unsigned long long* __restrict__ prep_bits,
                                                            unsigned long long* __restrict__ blk_pack8,
                                                            double* __restrict__ blk_dead8,
                                                            uint32_t* __restrict__ blk_ndead8, uint32_t part_base,
                                                            uint32_t part_stride,
                                                            const uint32_t* __restrict__ tile_list, uint32_t n_list,
                                                            uint32_t flags, unsigned long long* res_count) {
  // tiles [tile_lo, tile_hi) of one block of the sweep, two per trip, and behind them the n_list tiles of tile_list
  // (tiles of rows without in-edges that lie behind tile_hi), one per trip.  gs_mask: slots whose state writes the
  // current array in place (entry / in-place / flush, engine.hpp: GsState); entry_mask: those of them that add to what
  // it holds.  The tiles' classes (ApplyTileClass): a tile without in-edges gets the bits of every column, the columns
  // outside the sweep included (zeros), because the sweeps behind this one may not come by - also without kApplyLean,
  // where the kernel before the classes wrote only the active columns' words (zeros over zeros).  With kApplyLean in flags
  // a dead-end tile's rows are taken for what they are: no residue at a dense level, so it counts as 0
  // without the load; and no forward sweep leaves a contribution on them, so their lines of c8_next and c8_cur are
  // neither staged nor stored.  A backward call does leave one there (the entry preparation of a target without
  // out-edges), and only a store clears it: the launcher sets kApplyStoreDead for the forward sweeps behind a backward
  // one, which stage and store these tiles as plain ones.  Without kApplyLean a dead-end tile is a plain one.
  // res_count (hooks library, kApplyCountRes): [0] non-zero residues met on dead-end tiles, [1] residues loaded there,
  // [2] dead-end tiles an entry sweep came by.
  __shared__ double tile[kApplyGroups][kApplyRows][kBatch + 1];
  __shared__ uint32_t s_cls[kApplyGroups];
  __shared__ double tile_p[kApplyGroups][kApplyRows][kBatch + 1];  // what the rows leave in the current array (slots in gs_mask)
  __shared__ int32_t s_u[kApplyGroups][kApplyRows];
  __shared__ uint32_t s_d[kApplyGroups][kApplyRows];
  __shared__ uint32_t s_din[kApplyGroups][kApplyRows];  // backward sweeps: in-degree = edges the row pushes when it is popped
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the slot arguments load into SGPRs
  const uint32_t n_rows = n_nz + n_zin;
  const uint32_t n_tiles = (n_rows + kApplyRows - 1) / kApplyRows;
  SlotArgs a[kSlotsPerWave];
#pragma unroll
  for (int i = 0; i < kSlotsPerWave; ++i) a[i] = slots[w * kSlotsPerWave + i];
  double dead_next[kSlotsPerWave];
  unsigned long long pack[kSlotsPerWave];
  uint32_t ndead[kSlotsPerWave];
#pragma unroll
  for (int i = 0; i < kSlotsPerWave; ++i) {
    dead_next[i] = 0.0;
    pack[i] = 0;
    ndead[i] = 0;
  }
  // kApplyGroups tiles of 64 rows per trip (the waves of a workgroup spent four fifths of their cycles at the barriers
  // with one tile per trip).  A trip waits for memory three times: for its first phase's flight (ApplyFlight), for
  // the entry staging's loads, issued together, and for the residue / reserve loads of the wave's slots.
  const uint32_t pair_trips = tile_hi > tile_lo ? (tile_hi - tile_lo + kApplyGroups - 1) / kApplyGroups : 0u;
  for (uint32_t trip = blockIdx.x; trip < pair_trips + n_list; trip += gridDim.x) {
    // a listed tile travels alone: the trip's second tile counts as one behind the end
    const bool listed = trip >= pair_trips;
    const uint32_t tl0 = listed ? tile_list[trip - pair_trips] : tile_lo + trip * kApplyGroups;
    const uint32_t hi = listed ? tl0 + 1u : tile_hi;
    ApplyFlight f;
    apply_flight(f, tl0, n_nz, acc8, meta, cross_bits, tid);
#pragma unroll
    for (int g = 0; g < kApplyGroups; ++g) {
#pragma unroll
      for (int i = 0; i < kApplyPerThread; ++i) {
        const uint32_t idx = (uint32_t)i * (uint32_t)kApplyThreads + tid;
        const uint32_t r = idx / kBatch, s = idx % kBatch;
        // rows inside one 512-edge chunk are rewritten by plain stores every sweep; only the rows that
        // cross a chunk boundary are summed with atomics and have to be cleared for the next sweep
        const uint32_t j = (tl0 + g) * kApplyRows + r;
        const double v = (tl0 + g < hi && j < n_nz) ? f.v[g][i] : 0.0;  // (nothing looks at a value in flight)
        if (v != 0.0 && ((f.cw[g] >> r) & 1ull)) acc8[(size_t)j * kBatch + s] = 0.0;
        tile[g][r][s] = v;
      }
    }
    if (tid < kApplyRows * kApplyGroups) {
      const uint32_t g = tid / kApplyRows, r = tid % kApplyRows;
      const bool in = tl0 + g < hi;
      s_u[g][r] = in ? (int32_t)f.md.x : -1;
      s_d[g][r] = in ? f.md.y : 0u;
      s_din[g][r] = in ? f.md.z : 0u;
      if (r == 0) {
        uint32_t c = in ? f.md.w : (uint32_t)kTilePlain;
        if (c == kTileDeadEnd) c = !(flags & kApplyLean) ? (uint32_t)kTilePlain : ((flags & kApplyStoreDead) ? kTileDeadEndStored : c);
        s_cls[g] = c;
      }
    }
    __syncthreads();
    uint32_t cls[kApplyGroups];  // (the same for every thread: kept in SGPRs)
#pragma unroll
    for (int g = 0; g < kApplyGroups; ++g) cls[g] = __builtin_amdgcn_readfirstlane(s_cls[g]);
#ifdef PPRHIP_TEST_HOOKS
    if ((flags & kApplyCountRes) && entry_mask && tid == 0)
      for (int g = 0; g < kApplyGroups; ++g)
        if (cls[g] & 1u) atomicAdd(res_count + 2, 1ull);
#endif
    if (entry_mask) {  // entry sweeps add to the row's own pending contribution: stage it (whole lines)
      double p[kApplyGroups][kApplyPerThread];
#pragma unroll
      for (int g = 0; g < kApplyGroups; ++g) {
#pragma unroll
        for (int i = 0; i < kApplyPerThread; ++i) {
          const uint32_t idx = (uint32_t)i * (uint32_t)kApplyThreads + tid;
          const int32_t ur = s_u[g][idx / kBatch];
          p[g][i] = 0.0;  // (a dead-end tile's lines are zero and are not written below, unless kApplyStoreDead)
          if (cls[g] != kTileDeadEnd) p[g][i] = c8_cur[(size_t)(ur >= 0 ? ur : 0) * kBatch + idx % kBatch];  // (an absent row reads row 0)
        }
      }
#pragma unroll
      for (int g = 0; g < kApplyGroups; ++g) {
#pragma unroll
        for (int i = 0; i < kApplyPerThread; ++i) {
          const uint32_t idx = (uint32_t)i * (uint32_t)kApplyThreads + tid;
          const uint32_t r = idx / kBatch, s = idx % kBatch;
          tile_p[g][r][s] = (s_u[g][r] >= 0 && (entry_mask >> s & 1u)) ? p[g][i] : 0.0;
        }
      }
      __syncthreads();
    }
    // the wave's slots in three passes, so that all their residue / reserve loads are in flight together:
    // (1) row sums (+ the source's returned dead-end mass), (2) loads, (3) arithmetic and stores
    int32_t u[kApplyGroups];
    uint32_t d[kApplyGroups], din[kApplyGroups];
    double accv[kApplyGroups][kSlotsPerWave], oldv[kApplyGroups][kSlotsPerWave], rsvv[kApplyGroups][kSlotsPerWave];
    bool live[kApplyGroups][kSlotsPerWave];
#pragma unroll
    for (int g = 0; g < kApplyGroups; ++g) {
      u[g] = s_u[g][lane];
      d[g] = s_d[g][lane];
      din[g] = s_din[g][lane];
#pragma unroll
      for (int i = 0; i < kSlotsPerWave; ++i) {
        double acc = tile[g][lane][w * kSlotsPerWave + i];
        const bool on = a[i].active && u[g] >= 0;
        if (on && a[i].mode != kBackward && u[g] == a[i].src) {
          const double dd = a[i].ctr->dead[a[i].dead_slot];
          if (dd > 0.0) {
            acc += dd;
            a[i].ctr->dead[a[i].dead_slot] = 0.0;
          }
        } else if (a[i].seed_w && a[i].mode != kBackward) {
          // seed set (k_dense_apply's rule): the level's dead-end mass x lands on row u as x * seed_w[u].  The branch
          // is wave-uniform: a column that is not seeded loads nothing more.  x is one scalar load per wave, slot and
          // tile trip (held across the loop it cost more SGPR spills); the cell stays as it is - every block of a
          // Gauss-Seidel sweep reads it, k_seed_land_dense_batch clears it behind the last one.  A live seed without
          // in-edges needs no extra row: the sweep carries every row without in-edges that has out-edges (zin_rows).
          const double x = a[i].ctr->dead[a[i].dead_slot];
          if (x > 0.0 && on) {
            const double sw = a[i].seed_w[u[g]];
            if (sw != 0.0) acc += x * sw;
          }
        }
        accv[g][i] = acc;
        live[g][i] = on && acc > 0.0;
      }
    }
#pragma unroll
    for (int g = 0; g < kApplyGroups; ++g) {
#pragma unroll
      for (int i = 0; i < kSlotsPerWave; ++i) {
        // (a dead end that holds mass is in the frontier, so the level's preparation has taken it: zero without the load)
        oldv[g][i] = live[g][i] && !(cls[g] & 1u) ? slot_vec(a[i].res)[u[g]] : 0.0;
#ifdef PPRHIP_TEST_HOOKS
        if ((flags & kApplyCountRes) && (cls[g] & 1u) && live[g][i]) {  // load it all the same, and count
          oldv[g][i] = slot_vec(a[i].res)[u[g]];
          atomicAdd(res_count + 1, 1ull);
          if (oldv[g][i] != 0.0) atomicAdd(res_count, 1ull);
        }
#endif
        // (the reserve is needed when the row crosses, which most rows of a dense level do)
        rsvv[g][i] = live[g][i] ? slot_vec(a[i].reserve)[u[g]] : 0.0;
      }
    }
#pragma unroll
    for (int g = 0; g < kApplyGroups; ++g) {
#pragma unroll
      for (int i = 0; i < kSlotsPerWave; ++i) {
        const int s = w * kSlotsPerWave + i;
        double cn = 0.0;
        if (live[g][i] && a[i].mode == kBackward) {
          // Backward_Search.java:73-96 in pull form: the row's out-neighbours' (1 - alpha) * residue, divided by
          // this row's out-degree; strict un-normalised threshold
          const double old = oldv[g][i];
          const double nw = old + accv[g][i] / (double)d[g];
          if (!(old > a[i].rmax) && nw > a[i].rmax) {
            slot_vec(a[i].reserve)[u[g]] = rsvv[g][i] + nw * a[i].alpha;
            if (oldv[g][i] != 0.0) slot_vec(a[i].res)[u[g]] = 0.0;  // (rows that cross every sweep hold zero already)
            cn = (1.0 - a[i].alpha) * nw;
            pack[i] += (1ull << kPackShift) | (unsigned long long)din[g];
          } else {
            slot_vec(a[i].res)[u[g]] = nw;
          }
        } else if (live[g][i]) {
          const double old = oldv[g][i];
          const double nw = old + accv[g][i];
          bool crossing = !active_fwd(old, d[g], a[i].rmax) && active_fwd(nw, d[g], a[i].rmax);
          if (a[i].mode == kFwdTopk) {
            if (a[i].rmax < a[i].min_rmax && active_fwd(old, d[g], a[i].rmax)) crossing = take_armed_slot(a[i].armed, u[g]);
            if (active_fwd(nw, d[g], a[i].min_rmax)) slot_vec(a[i].flags)[u[g]] = 1;
          }
          if (crossing) {  // becomes a frontier node of the next level: prepare it right here
            slot_vec(a[i].reserve)[u[g]] = rsvv[g][i] + nw * a[i].alpha;
            if (oldv[g][i] != 0.0) slot_vec(a[i].res)[u[g]] = 0.0;  // (rows that cross every sweep hold zero already)
            if (d[g] == 0) {
              dead_next[i] += nw * (1.0 - a[i].alpha);
              ndead[i]++;
            } else {
              cn = ((1.0 - a[i].alpha) * nw) / (double)d[g];
            }
            pack[i] += (1ull << kPackShift) | (unsigned long long)d[g];
          } else {
            slot_vec(a[i].res)[u[g]] = nw;
          }
        }
        tile[g][lane][s] = cn;
        if (gs_mask >> s & 1u) {
          const int gst = a[i].gs_state;
          // entry: old + new (the old value was staged in tile_p above)
          tile_p[g][lane][s] = gst == kGsEntry ? tile_p[g][lane][s] + cn : (gst == kGsInPlace ? cn : 0.0);
        }
        // rows of this tile that hold a contribution for the slot's next level (read when the slot
        // goes back to list form)
        const unsigned long long bits = (cls[g] & 1u) ? 0ull : __ballot(cn > 0.0);
        const bool wr = a[i].active || cls[g] == kTileNoIn;  // (a column outside the sweep has cn = 0 everywhere)
        if (lane == 0 && wr && tl0 + g < hi) prep_bits[(size_t)s * n_tiles + tl0 + g] = bits;
      }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kApplyGroups; ++g) {
      if (cls[g] == kTileDeadEnd) continue;  // zeros over zeros (kTileDeadEndStored: over what a backward call left)
#pragma unroll
      for (int i = 0; i < kApplyPerThread; ++i) {
        const uint32_t idx = (uint32_t)i * (uint32_t)kApplyThreads + tid;
        const uint32_t r = idx / kBatch, s = idx % kBatch;
        const int32_t ur = s_u[g][r];
        if (ur >= 0) {
          c8_next[(size_t)ur * kBatch + s] = tile[g][r][s];
          if (gs_mask >> s & 1u) c8_cur[(size_t)ur * kBatch + s] = tile_p[g][r][s];
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < kSlotsPerWave; ++i) {
    const double ds = wave_sum_f64(dead_next[i]);
    const unsigned long long ps = wave_sum_u64(pack[i]);
    const unsigned long long nd = wave_sum_u64((unsigned long long)ndead[i]);
    if (lane == 0) {
      const size_t o = (size_t)(w * kSlotsPerWave + i) * part_stride + part_base + blockIdx.x;
      blk_pack8[o] = ps;
      blk_dead8[o] = ds;
      blk_ndead8[o] = (uint32_t)nd;
    }
  }
}

// workgroup s sums slot s's partials into that slot's counters
__global__ __launch_bounds__(1024) void k_dense_reduce_batch(const unsigned long long* __restrict__ blk_pack8,
                                                           const double* __restrict__ blk_dead8,
                                                           const uint32_t* __restrict__ blk_ndead8, uint32_t n_blocks,
                                                           uint32_t part_stride,
                                                           const SlotArgs* __restrict__ slots,
                                                           unsigned long long* __restrict__ sweep_out) {
  __shared__ double s_red[16];
  __shared__ unsigned long long s_red2[16];
  const SlotArgs a = slots[blockIdx.x];
  if (!a.active) return;
  unsigned long long pack = 0, ndead = 0;
  double dead = 0.0;
  for (uint32_t i = threadIdx.x; i < n_blocks; i += blockDim.x) {
    pack += blk_pack8[(size_t)blockIdx.x * part_stride + i];
    dead += blk_dead8[(size_t)blockIdx.x * part_stride + i];
    ndead += blk_ndead8[(size_t)blockIdx.x * part_stride + i];
  }
  const unsigned long long ps = block_sum_u64(pack, s_red2);
  const unsigned long long nd = block_sum_u64(ndead, s_red2);
  const double ds = block_sum_f64(dead, s_red);
  if (threadIdx.x == 0) {
    a.ctr->packed[a.out_slot] = ps;
    sweep_out[blockIdx.x] = ps;  // all slots' new frontier counters side by side: one read-back per sweep
    if (nd) {
      a.ctr->dead[a.dead_slot ^ 1] = a.ctr->dead[a.dead_slot ^ 1] + ds;
      a.ctr->dead_pops += nd;
    }
  }
}

// The same for the seeded columns of a batched sweep, all in one launch (blockIdx.y = column), between the last apply
// block and k_dense_reduce_batch: column c's dead-end seeds take x e_j and its cell is cleared (the workspace's own
// SeedTable::done counts the column's workgroups).  Columns that are not seeded or not in the sweep return at once.
__global__ __launch_bounds__(256) void k_seed_land_dense_batch(const SlotArgs* __restrict__ slots) {
  const SlotArgs& a = slots[blockIdx.y];
  if (!a.active || !a.seed_w || a.mode == kBackward) return;
  const double x = a.ctr->dead[a.dead_slot];
  if (!(x > 0.0)) return;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = a.seed_n_live + blockIdx.x * blockDim.x + threadIdx.x; i < a.seed_n_all; i += stride)
    a.reserve[a.seed_id[i]] = a.reserve[a.seed_id[i]] + x * a.seed_e[i];
  seed_land_done(a.seed_done, a.ctr, a.dead_slot);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// LDS table of the batched edge kernel.  PPRHIP_SWEEP_HOT_KB (measurement switch): its size in KB, at most 128.
static uint32_t sweep_hot_bytes() {
  static const uint32_t v = [] {
    const char* e = hook_env("PPRHIP_SWEEP_HOT_KB");
    const long kb = e ? atol(e) : 0;
    return kb >= 0 && e && kb * 1024 <= kHotBytes ? (uint32_t)(kb * 1024) : (uint32_t)kHotDefaultBytes;
  }();
  return v;
}

template <int G>
static int launch_dense_edges_bG(pprhip_graph* g, const int32_t* ci, const uint8_t* start_flags,
                                 const uint32_t* chunk_starts, const double* cB, double* accB, const GsBlock& B) {
  if (!g->gr->n_chunks || B.e_hi <= B.e_lo) return PPRHIP_OK;
  const uint32_t hot_max = sweep_hot_bytes() / (8 * G);
  const uint32_t n_hot = g->gr->relabeled ? std::min<uint32_t>(g->gr->n, hot_max) : 0u;
  const uint32_t c_lo = (uint32_t)(B.e_lo / kChunkEdges);
  const uint32_t c_hi = (uint32_t)((B.e_hi + kChunkEdges - 1) / kChunkEdges);
  const uint32_t want = (c_hi - c_lo + 15) / 16;
  const unsigned long long* flags64 = reinterpret_cast<const unsigned long long*>(start_flags);
  if (n_hot) {
    const uint32_t grid = std::min<uint32_t>(want, (uint32_t)g->gr->n_cus);
    k_dense_edges_b<true, G><<<dim3(grid), dim3(1024), sizeof(double) * n_hot * G, g->stream>>>(
        ci, flags64, chunk_starts, c_hi, (unsigned long long)g->gr->m, cB, accB, n_hot, c_lo, B.e_lo, B.e_hi, g->gr->n);
  } else {
    const uint32_t grid = std::min<uint32_t>(want, (uint32_t)g->gr->n_cus * 2u);
    k_dense_edges_b<false, G><<<dim3(grid), dim3(1024), 0, g->stream>>>(
        ci, flags64, chunk_starts, c_hi, (unsigned long long)g->gr->m, cB, accB, 0u, c_lo, B.e_lo, B.e_hi, g->gr->n);
  }
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

#ifdef PPRHIP_TEST_HOOKS
// measurement (PPRHIP_COUNT_LIVE): how many of a sweep's gathers fetch a line that is zero in every column?
// out[0] += out-degrees of the nodes whose line holds a non-zero, out[1] += such nodes
__global__ __launch_bounds__(256) void k_count_live_lines(const double* __restrict__ c8, const uint32_t* __restrict__ out_rp,
                                                          uint32_t n, unsigned long long* out) {
  __shared__ unsigned long long s_red[4];
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  unsigned long long d = 0, c = 0;
  if (v < n) {
    bool live = false;
    for (int s = 0; s < kBatch; ++s) live |= c8[(size_t)v * kBatch + s] != 0.0;
    if (live) {
      d = out_rp[v + 1] - out_rp[v];
      c = 1;
    }
  }
  const unsigned long long ds = block_sum_u64(d, s_red), cs = block_sum_u64(c, s_red);
  if (threadIdx.x == 0 && (ds | cs)) {
    atomicAdd(&out[0], ds);
    atomicAdd(&out[1], cs);
  }
}
int launch_count_live_lines(pprhip_graph* P, unsigned long long* d_out) {
  const BatchState* bs = P->batch;
  k_count_live_lines<<<dim3((P->gr->n + 255) / 256), dim3(256), 0, P->stream>>>(bs->c8[bs->c8cur], P->gr->out_rp, P->gr->n,
                                                                              d_out);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// the edge kernel of one block of a batched forward sweep alone (pprhip_hook_time_sweep_edges)
int launch_sweep_edges_only(pprhip_graph* P, const GsBlock& B) {
  const GraphData* D = P->gr;
  const BatchState* bs = P->batch;
  return launch_dense_edges_bG<kBatch>(P, D->in_ci, D->start_flags, D->chunk_starts, bs->c8[bs->c8cur], bs->acc8, B);
}
#endif

int launch_build_apply_meta(pprhip_graph* P, bool backward) {
  const GraphData* D = P->gr;
  const SweepSide S = sweep_side(D, backward);
  const uint32_t n_pad = (uint32_t)apply_meta_rows(S.n_nz + S.n_z);
  k_build_apply_meta<<<dim3((n_pad + 255) / 256), dim3(256), 0, P->stream>>>(
      S.nz_rows, S.n_nz, S.z_rows, S.n_z, D->out_rp, backward ? D->in_rp : nullptr, P->batch->apply_meta[backward], n_pad);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

static_assert(kApplyRows * kApplyGroups == 128, "apply_meta_rows (engine.hpp) pads the records to pairs of 64-row tiles");
static_assert(kApplyRows == kTileRows, "launch_compact_prepared (kernels_frontier.hip) finds a slot's prep_bits by kTileRows");

int launch_dense_level_b8(pprhip_graph* P, bool backward, const GsBlock* gs_blocks, int n_gs_blocks) {
  const GraphData* D = P->gr;
  BatchState* bs = P->batch;
  const SweepSide S = sweep_side(D, backward);
  const uint4* meta = bs->apply_meta[backward];
  if (!meta) {
    set_error("batched sweep: no row records for the %s side", backward ? "backward" : "forward");
    return PPRHIP_ERR_INVALID;
  }
  // slots whose sweep state writes the current contribution array in place; without any, one launch serves the
  // whole sweep (Jacobi rows do not care in which order the blocks run)
  uint32_t gs_mask = 0, entry_mask = 0;
  for (int s = 0; s < kBatch; ++s)
    if (bs->h_slot_args[s].active) {
      const int st = bs->h_slot_args[s].gs_state;
      if (st == kGsEntry || st == kGsInPlace || st == kGsFlush) gs_mask |= 1u << s;
      if (st == kGsEntry) entry_mask |= 1u << s;
    }
  const uint32_t n_rows = S.n_nz + S.n_z;
  const uint32_t n_tiles = (n_rows + kApplyRows - 1) / kApplyRows;
  const GsBlock whole{0u, S.n_nz, 0ull, (unsigned long long)D->m};
  const bool cut = gs_mask && gs_blocks && n_gs_blocks > 1 && !backward;
  const GsBlock* blocks = cut ? gs_blocks : &whole;
  const int nb = cut ? n_gs_blocks : 1;
  // seed sets: the dead-end seeds of every seeded column (landed behind the last apply block)
  uint32_t seed_dead_max = 0;
  bool seeded = false;
  for (int s = 0; s < kBatch; ++s) {
    const SlotArgs& sa = bs->h_slot_args[s];
    if (sa.active && sa.seed_w && !backward) {
      seeded = true;
      seed_dead_max = std::max(seed_dead_max, sa.seed_n_all - sa.seed_n_live);
    }
  }
  // Rows the apply skips.  The tiles from z_lo on hold rows without in-edges only: their row sums are 0
  // by construction, so a column is live there on the row of its source alone (returned dead-end mass), and what a
  // sweep would write everywhere else - zeros into the array it fills, zero bits - is there already.  The sweep visits
  // the tiles of its columns' sources and those of the two sweeps before (the arrays ping-pong: an entry written in
  // sweep k sits in the array that sweep k + 2 fills again; a column's bits are rewritten by the next sweep that comes
  // by, whether the column is in it or not).  A seeded column lands mass on any row, a backward sweep has another
  // layout and without the relabeling a row's ordinal is not its node: such a sweep and the two behind it run over
  // every tile, as the first two of a batch state do.  Those sweeps also stage and store the dead-end tiles
  // (kApplyStoreDead): the entry preparation of a backward call leaves a contribution on a target without out-edges,
  // in the array its sweep reads, and the call may end before a backward sweep has filled that array again.  The first
  // forward sweep behind it does, as every forward sweep did before the classes.  PPRHIP_APPLY_ALL_ROWS=1 (test
  // switch, read at every launch): every tile, every load and every store, as before the classes - but for the bits
  // of the columns outside the sweep on tiles without in-edges, which are written all the same (zeros over zeros).
  const char* const all_rows_env = hook_env("PPRHIP_APPLY_ALL_ROWS");
  const bool all_rows = all_rows_env && all_rows_env[0] == '1';
  const uint32_t z_lo = (S.n_nz + kApplyRows - 1) / kApplyRows;
  uint32_t now[kBatch];
  int n_now = 0;
  auto add_unique = [](uint32_t* v, int& n, uint32_t t) {
    for (int i = 0; i < n; ++i)
      if (v[i] == t) return;
    v[n++] = t;
  };
  if (backward || seeded || !D->relabeled) {
    bs->zin_full_left = 3;
  } else {
    for (int s = 0; s < kBatch; ++s) {
      const SlotArgs& sa = bs->h_slot_args[s];
      if (!sa.active || sa.src < 0) continue;
      const uint32_t t = (uint32_t)sa.src / kApplyRows;  // (relabeled: a row's ordinal is its node)
      if (t >= z_lo && t < n_tiles) add_unique(now, n_now, t);
    }
  }
  const bool full = all_rows || bs->zin_full_left > 0;
  if (bs->zin_full_left > 0) bs->zin_full_left--;
  uint32_t* list = reinterpret_cast<uint32_t*>(bs->h_slot_args + kBatch);
  int n_list = 0;
  if (!full) {
    for (int i = 0; i < n_now; ++i) add_unique(list, n_list, now[i]);
    for (int h = 0; h < 2; ++h)
      for (int i = 0; i < bs->zin_hist_n[h]; ++i) add_unique(list, n_list, bs->zin_hist[h][i]);
  }
  std::copy(bs->zin_hist[0], bs->zin_hist[0] + bs->zin_hist_n[0], bs->zin_hist[1]);
  bs->zin_hist_n[1] = bs->zin_hist_n[0];
  std::copy(now, now + n_now, bs->zin_hist[0]);
  bs->zin_hist_n[0] = n_now;
  // the slots' arguments and the tile list in one block: no further command on the sweep's stream
  PPRHIP_CHECK_HIP(hipMemcpyAsync(bs->d_slot_args, bs->h_slot_args, slot_args_bytes(), hipMemcpyHostToDevice, P->stream));
  const uint32_t* d_list = reinterpret_cast<const uint32_t*>(bs->d_slot_args + kBatch);
  uint32_t flags = all_rows ? 0u : (full ? kApplyLean | kApplyStoreDead : kApplyLean);
  unsigned long long* res_count = nullptr;
#ifdef PPRHIP_TEST_HOOKS
  // PPRHIP_APPLY_COUNT_RES=1 (test switch): the residues of dead-end tiles are loaded all the same and the non-zero ones
  // counted (batch_run hands the count out in the call's statistics)
  res_count = bs->apply_res_count;
  if (hook_env("PPRHIP_APPLY_COUNT_RES") && flags) flags |= kApplyCountRes;
#endif
  uint32_t part_base = 0;
  for (int b = 0; b < nb; ++b) {
    const GsBlock& B = blocks[b];
    const bool last = b == nb - 1;
    PPRHIP_TRY(launch_dense_edges_bG<kBatch>(P, S.ci, S.start_flags, S.chunk_starts, bs->c8[bs->c8cur], bs->acc8, B));
    // block boundaries are multiples of 256 row ordinals, so tiles never straddle; the rows without in-edges
    // follow the last block.  The last block's rows are read by nobody again in this sweep (the next sweep reads the
    // other array), so only the blocks before it write the current array in place.
    const uint32_t t_lo = B.j_lo / kApplyRows;
    const uint32_t t_hi = last ? (full ? n_tiles : z_lo) : B.j_hi / kApplyRows;
    const uint32_t nl = last && !full ? (uint32_t)n_list : 0u;
    const uint32_t trips = (t_hi > t_lo ? (t_hi - t_lo + kApplyGroups - 1) / kApplyGroups : 0u) + nl;
    if (!trips) continue;
    const uint32_t quota = kApplyBlocks8 / (uint32_t)nb;
    uint32_t grid = std::max(1u, std::min(trips, quota));
    // PPRHIP_APPLY_GRID (test switch, read at every launch): at most so many workgroups, so that a graph of a few
    // hundred rows gives a workgroup a second and a third trip
    if (const char* e = hook_env("PPRHIP_APPLY_GRID"))
      if (atol(e) > 0) grid = (uint32_t)std::min<long>(grid, atol(e));
    k_dense_apply_batch<<<dim3(grid), dim3(kApplyThreads), 0, P->stream>>>(
          meta, S.n_nz, S.n_z, bs->acc8, bs->c8[bs->c8cur],
          bs->c8[bs->c8cur ^ 1], t_lo, t_hi, last ? 0u : gs_mask, last ? 0u : entry_mask, bs->d_slot_args,
          S.cross_bits, bs->prep_bits, bs->blk_pack8, bs->blk_dead8, bs->blk_ndead8, part_base, kApplyBlocks8, d_list, nl,
          flags, res_count);
    PPRHIP_CHECK_HIP(hipGetLastError());
    part_base += grid;
  }
  if (seeded) {
    k_seed_land_dense_batch<<<dim3(grid_for(seed_dead_max, 256, 1024), kBatch), dim3(256), 0, P->stream>>>(
        bs->d_slot_args);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  k_dense_reduce_batch<<<dim3(kBatch), dim3(1024), 0, P->stream>>>(bs->blk_pack8, bs->blk_dead8, bs->blk_ndead8, part_base,
                                                                   kApplyBlocks8, bs->d_slot_args, bs->sweep_out);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// Current device: code object loaded, the edge kernel's LDS table opted in (see init_kernels_push).
int init_kernels_dense_batch() {
  PPRHIP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dense_edges_b<true, kBatch>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kHotBytes));
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_dense_apply_batch)));
  return PPRHIP_OK;
}

}  // namespace pprhip
