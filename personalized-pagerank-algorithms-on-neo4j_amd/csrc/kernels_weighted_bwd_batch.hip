// kernels_weighted_bwd_batch.hip — the dense level of sixteen WEIGHTED BACKWARD pushes at once for gfx950 (MI355X):
// the batched sweep of kernels_weighted_batch.hip over the other CSR (DESIGN.md §2 "Batched weighted targets";
// weighted_bwd_batch.cpp drives them).  The contributions c(v) = (1 - alpha) r(v) of the kBatch pushes in flight are
// interleaved, c8[v][column] - one 128-byte line per vertex - in the batch state's arrays, the row sums in
// acc8[out-row ordinal][column]; residue and reserve stay the slots' own vectors (SlotArgs).
//
//   k_wbb_edges    k_wbat_edges over out_ci / out_w: a wave owns a chunk of 512 out-edges, both streams are read once,
//                  non-temporally, 8 edges per lane; G = 16 lanes (one per column) share an edge, lane group g walks edges
//                  [128 g, 128 (g + 1)) of the chunk; an edge's index and weight come out of the owning lane's registers
//                  with ds_swizzle, the gather brings the line c8[dst][0..15], the term is c8[dst][column] * w(e) - the
//                  product k_wb_edges forms.  Only rows that cross the chunk boundary use atomics on acc8.  No LDS.
//                  out_w holds exactly m weights (in_w is padded, out_w is not): a lane whose 8 edges reach beyond m reads
//                  its weights one by one, 0.0 for a padding edge, as wb_load_chunk does.
//   k_wbb_apply    k_wb_dense_apply per (row, column): 64 rows at a time through an LDS tile [row][column], so that acc8
//                  and c8 move as whole lines while a wave walks a column's residue / reserve with a lane per row.  The
//                  row sum is divided by W(u) once, lands, and a crossing row (!(old > rmax) && new > rmax) is prepared in
//                  place with its in-degree.  An idle column gets zeros.  No dead-end mass, no source row.
//   k_wbb_reduce   the per-workgroup partials of every column into the slot's counter and into sweep_out.
//   k_wbb_scatter  k_wb_prepare writing c with stride kBatch: a slot's frontier list enters its column.
//   k_wbb_compact  a column back to list form, weighted by the in-degree (and handed back all-zero):
//                  launch_compact_prepared(..., backward) for cdense.
//   k_wbb_leave    the scattered list's members without out-edges - rows k_wbb_apply never rewrites - zeroed in both
//                  arrays once the first sweep has consumed them (the serial path's memset after a phase's first level).
//
// All arithmetic is IEEE double with -ffp-contract=off, a term is c * w(e), a row's sum is divided by W(u) once:
// batching changes the order of additions inside dense levels and nothing else (tests/weighted_bwd_ref.py).
#include "weighted_device.hpp"

namespace pprhip {

constexpr int kWbbG = kBatch;  // lanes per edge = columns
static_assert(kWbbG == 16, "the lane groups of k_wbb_edges and the flag words they read are laid out for sixteen columns");
// A chunk's row-start bits are read as 64-bit words: chunk c, lane group g reads words 8 c + 2 g and 8 c + 2 g + 1, the
// last one ends at byte 64 (c + 1) <= 64 n_chunks, inside the (n_chunks + 1) * 64 bytes ensure_bwd_layout allocates.
static_assert(kChunkEdges / 8 == 64 && (64 / kWbbG) * 2 * 8 == kChunkEdges / 8, "flag words of a chunk");

// value of lane K of the caller's lane group of 16
template <int K>
__device__ __forceinline__ int wbb_bcast(int x) {
  return __builtin_amdgcn_ds_swizzle(x, (0x1f & ~(kWbbG - 1)) | (K << 5));
}
template <int K>
__device__ __forceinline__ double wbb_bcast_f64(double x) {
  return __hiloint2double(wbb_bcast<K>(__double2hiint(x)), wbb_bcast<K>(__double2loint(x)));
}

struct WbbChunkRegs {  // one lane's share of a chunk: 8 indices, their weights; the row-start bits of its group's 128 edges
  int4 ia, ib;
  double w[8];
  unsigned long long mask[2];
};

__device__ __forceinline__ WbbChunkRegs wbb_load_chunk(const int32_t* __restrict__ out_ci, const double* __restrict__ out_w,
                                                     unsigned long long m, const unsigned long long* __restrict__ flags64,
                                                     uint32_t c, int lane) {
  const unsigned long long e0 = (unsigned long long)c * kChunkEdges + 8ull * lane;
  // both streams are read once per sweep: non-temporal, so that they do not push gathered lines out of L2
  typedef int v4i __attribute__((ext_vector_type(4)));
  typedef double v2d __attribute__((ext_vector_type(2)));
  const v4i* q = reinterpret_cast<const v4i*>(out_ci + e0);  // (out_ci is padded to whole chunks with index 0)
  const v4i x = __builtin_nontemporal_load(q), y = __builtin_nontemporal_load(q + 1);
  WbbChunkRegs r;
  r.ia = make_int4(x.x, x.y, x.z, x.w);
  r.ib = make_int4(y.x, y.y, y.z, y.w);
  if (e0 + 8ull <= m) {
    const v2d* qw = reinterpret_cast<const v2d*>(out_w + e0);
    const v2d w0 = __builtin_nontemporal_load(qw), w1 = __builtin_nontemporal_load(qw + 1),
              w2 = __builtin_nontemporal_load(qw + 2), w3 = __builtin_nontemporal_load(qw + 3);
    r.w[0] = w0.x; r.w[1] = w0.y; r.w[2] = w1.x; r.w[3] = w1.y;
    r.w[4] = w2.x; r.w[5] = w2.y; r.w[6] = w3.x; r.w[7] = w3.y;
  } else {  // the last chunk: no load past out_w[m)
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = e0 + i < m ? out_w[e0 + i] : 0.0;
  }
  const size_t f0 = (size_t)c * 8 + (size_t)(lane / kWbbG) * 2;
  r.mask[0] = __builtin_nontemporal_load(&flags64[f0]);
  r.mask[1] = __builtin_nontemporal_load(&flags64[f0 + 1]);
  return r;
}

// 8 edges of the group: their indices and weights sit in lane JB of the group
template <int JB>
__device__ __forceinline__ void wbb_edges_block(const WbbChunkRegs& cur, const double* __restrict__ cB, int s, uint32_t before,
                                              double* __restrict__ accB, double& seg, double& first_seg, uint32_t& k) {
  const int32_t own[8] = {cur.ia.x, cur.ia.y, cur.ia.z, cur.ia.w, cur.ib.x, cur.ib.y, cur.ib.z, cur.ib.w};
  uint32_t v[8];
  double w[8], val[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (uint32_t)wbb_bcast<JB>(own[i]);
#pragma unroll
  for (int i = 0; i < 8; ++i) val[i] = cB[(size_t)v[i] * kWbbG + s];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = wbb_bcast_f64<JB>(cur.w[i]);
#pragma unroll
  for (int i = 0; i < 8; ++i) val[i] = val[i] * w[i];  // (a padding edge: destination 0, weight 0.0)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if ((cur.mask[(JB * 8 + i) >> 6] >> ((JB * 8 + i) & 63)) & 1ull) {
      if (k == 0)
        first_seg = seg;  // closes the row carried in from earlier groups
      else
        __builtin_nontemporal_store(seg, &accB[(size_t)(before + k - 1) * kWbbG + s]);  // starts and ends inside this group
      seg = 0.0;
      ++k;
    }
    seg += val[i];
  }
}

template <int JB>
struct WbbEdgeBlocks {
  static __device__ __forceinline__ void run(const WbbChunkRegs& cur, const double* __restrict__ cB, int s, uint32_t before,
                                             double* __restrict__ accB, double& seg, double& first_seg, uint32_t& k) {
    WbbEdgeBlocks<JB - 1>::run(cur, cB, s, before, accB, seg, first_seg, k);
    wbb_edges_block<JB>(cur, cB, s, before, accB, seg, first_seg, k);
  }
};
template <>
struct WbbEdgeBlocks<-1> {
  static __device__ __forceinline__ void run(const WbbChunkRegs&, const double*, int, uint32_t, double*, double&, double&,
                                             uint32_t&) {}
};

// ------------------------------------------------------------------------------------------------
// the batched weighted backward sweep: edges
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_wbb_edges(const int32_t* __restrict__ out_ci, const double* __restrict__ out_w,
                                                  unsigned long long m, const unsigned long long* __restrict__ flags64,
                                                  const uint32_t* __restrict__ chunk_starts, uint32_t n_chunks,
                                                  const double* __restrict__ cB, double* __restrict__ accB) {
  const int lane = lane_id();
  const int grp = lane / kWbbG, s = lane & (kWbbG - 1);
  const uint32_t waves_per_block = blockDim.x >> 6;
  const uint32_t stride = gridDim.x * waves_per_block;
  uint32_t c = blockIdx.x * waves_per_block + (uint32_t)__builtin_amdgcn_readfirstlane(wave_id());
  if (c >= n_chunks) return;
  WbbChunkRegs cur = wbb_load_chunk(out_ci, out_w, m, flags64, c, lane);
  for (; c < n_chunks; c += stride) {
    // the next chunk's streams are requested before this chunk's gathers, so their latency is hidden
    WbbChunkRegs nxt = cur;
    if (c + stride < n_chunks) nxt = wbb_load_chunk(out_ci, out_w, m, flags64, c + stride, lane);
    const uint32_t cs = chunk_starts[c];
    const uint32_t pc = (uint32_t)__popcll(cur.mask[0]) + (uint32_t)__popcll(cur.mask[1]);
    const uint32_t incl = wave_incl_scan_u32_dpp(s == 0 ? pc : 0u);  // row starts up to and including this group
    const uint32_t before = cs + incl - pc;
    double seg = 0.0, first_seg = 0.0;
    uint32_t k = 0;
    WbbEdgeBlocks<kWbbG - 1>::run(cur, cB, s, before, accB, seg, first_seg, k);
    // segmented scan over the lane groups: S(g) = tail(g) + (group g holds a row start ? 0 : S(g-1))
    const bool h = k != 0;
    double S = seg;
    int F = h ? 1 : 0;
#pragma unroll
    for (int d = kWbbG; d < 64; d <<= 1) {
      const double ps = __shfl_up(S, d);
      const int pf = __shfl_up(F, d);
      if (lane >= d) {
        if (!F) S += ps;
        F |= pf;
      }
    }
    double carry = __shfl_up(S, kWbbG);
    if (lane < kWbbG) carry = 0.0;
    const unsigned long long hmask = __ballot(h);
    if (h) {
      // the row that ends at this group's first start flag: edges carried in + this group's head
      const bool nonempty = grp > 0 || (cur.mask[0] & 1ull) == 0;
      if (nonempty && before > 0) {
        const double total = carry + first_seg;
        const bool started_here = (hmask & ((1ull << (grp * kWbbG)) - 1ull)) != 0;  // an earlier group starts a row
        double* dst = &accB[(size_t)(before - 1) * kWbbG + s];
        if (started_here)
          *dst = total;
        else
          atomic_add_noret(dst, total);  // began in an earlier chunk
      }
    }
    if (grp == 64 / kWbbG - 1) {  // the row still open at the end of the chunk
      const uint32_t starts = cs + incl;
      if (starts > 0 && S != 0.0) atomic_add_noret(&accB[(size_t)(starts - 1) * kWbbG + s], S);
    }
    cur = nxt;
  }
}

// ------------------------------------------------------------------------------------------------
// the batched weighted backward sweep: apply
// ------------------------------------------------------------------------------------------------
constexpr int kWbbRows = 64;       // rows of a tile
constexpr int kWbbThreads = 256;   // 4 waves, 4 columns each
constexpr int kWbbSlotsPerWave = kBatch / (kWbbThreads / 64);
constexpr int kWbbPerThread = kWbbRows * kBatch / kWbbThreads;

// k_wb_dense_apply's row: the row sum `acc` of row u is divided by W(u), lands, the backward threshold is tested and a
// crossing row is prepared in place.  Returns c_next[u][column].
__device__ __forceinline__ double wbb_apply_row(const SlotArgs& a, int32_t u, double acc, double Wu,
                                              const uint32_t* __restrict__ in_rp, unsigned long long& pack) {
  double cn = 0.0;
  if (acc > 0.0) {
    const double add = acc / Wu;
    const double old = a.res[u];
    const double nw = old + add;
    if (!(old > a.rmax) && nw > a.rmax) {  // becomes a frontier node of the next level: prepare it right here
      a.reserve[u] = a.reserve[u] + nw * a.alpha;
      if (old != 0.0) a.res[u] = 0.0;
      cn = (1.0 - a.alpha) * nw;
      pack += (1ull << kPackShift) | (unsigned long long)(in_rp[u + 1] - in_rp[u]);
    } else {
      a.res[u] = nw;
    }
  }
  return cn;
}

__global__ __launch_bounds__(kWbbThreads) void k_wbb_apply(const int32_t* __restrict__ nz_rows, uint32_t n_nz,
                                                         double* __restrict__ acc8, const uint32_t* __restrict__ in_rp,
                                                         const double* __restrict__ wsum, double* __restrict__ c8_next,
                                                         const SlotArgs* __restrict__ slots,
                                                         unsigned long long* __restrict__ blk_pack8, uint32_t part_stride) {
  __shared__ double tile[kWbbRows][kBatch + 1];
  __shared__ int32_t s_u[kWbbRows];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the slot arguments load into SGPRs
  SlotArgs a[kWbbSlotsPerWave];
  unsigned long long pack[kWbbSlotsPerWave];
#pragma unroll
  for (int i = 0; i < kWbbSlotsPerWave; ++i) {
    a[i] = slots[w * kWbbSlotsPerWave + i];
    pack[i] = 0ull;
  }
  const uint32_t n_tiles = (n_nz + kWbbRows - 1) / kWbbRows;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t j0 = t * kWbbRows;
    // the tile's row sums come in as whole lines; every entry met non-zero is cleared (the rows that cross a chunk
    // boundary are summed with atomics, the others are rewritten by plain stores every sweep)
#pragma unroll
    for (int i = 0; i < kWbbPerThread; ++i) {
      const uint32_t idx = (uint32_t)i * (uint32_t)kWbbThreads + tid;
      const uint32_t r = idx / kBatch, s = idx % kBatch, j = j0 + r;
      double v = 0.0;
      if (j < n_nz) {
        v = acc8[(size_t)j * kBatch + s];
        if (v != 0.0) acc8[(size_t)j * kBatch + s] = 0.0;
      }
      tile[r][s] = v;
    }
    if (tid < kWbbRows) s_u[tid] = j0 + tid < n_nz ? nz_rows[j0 + tid] : -1;
    __syncthreads();
    const int32_t u = s_u[lane];
    const double Wu = u >= 0 ? wsum[u] : 1.0;  // (a row with out-edges: W(u) > 0)
#pragma unroll
    for (int i = 0; i < kWbbSlotsPerWave; ++i) {
      const int s = w * kWbbSlotsPerWave + i;
      double cn = 0.0;
      if (a[i].active && u >= 0) cn = wbb_apply_row(a[i], u, tile[lane][s], Wu, in_rp, pack[i]);
      tile[lane][s] = cn;  // (an idle column: zeros)
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kWbbPerThread; ++i) {
      const uint32_t idx = (uint32_t)i * (uint32_t)kWbbThreads + tid;
      const uint32_t r = idx / kBatch, s = idx % kBatch;
      const int32_t ur = s_u[r];
      if (ur >= 0) c8_next[(size_t)ur * kBatch + s] = tile[r][s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < kWbbSlotsPerWave; ++i) {
    const unsigned long long ps = wave_sum_u64(pack[i]);
    // per-workgroup partials, one per wave's column: k_wbb_reduce sums them (no same-address atomics in this kernel)
    if (lane == 0) blk_pack8[(size_t)(w * kWbbSlotsPerWave + i) * part_stride + blockIdx.x] = ps;
  }
}

// workgroup s sums column s's partials into that slot's counter (k_wbat_reduce without the dead-end cells)
__global__ __launch_bounds__(1024) void k_wbb_reduce(const unsigned long long* __restrict__ blk_pack8, uint32_t n_blocks,
                                                   uint32_t part_stride, const SlotArgs* __restrict__ slots,
                                                   unsigned long long* __restrict__ sweep_out) {
  __shared__ unsigned long long s_red2[16];
  const SlotArgs a = slots[blockIdx.x];
  if (!a.active) return;
  unsigned long long pack = 0;
  for (uint32_t i = threadIdx.x; i < n_blocks; i += blockDim.x) pack += blk_pack8[(size_t)blockIdx.x * part_stride + i];
  const unsigned long long ps = block_sum_u64(pack, s_red2);
  if (threadIdx.x == 0) {
    a.ctr->packed[a.out_slot] = ps;
    sweep_out[blockIdx.x] = ps;
  }
}

// ------------------------------------------------------------------------------------------------
// entering and leaving a column
// ------------------------------------------------------------------------------------------------
// k_wb_prepare with the contributions written into column `col` of the interleaved array (all-zero beforehand)
__global__ __launch_bounds__(256) void k_wbb_scatter(const int32_t* __restrict__ F, uint32_t nf, double* __restrict__ res,
                                                    double* __restrict__ reserve, double* __restrict__ c8, uint32_t col,
                                                    double alpha) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
    const int32_t v = F[i];
    const double rc = res[v];
    res[v] = 0.0;
    reserve[v] = reserve[v] + rc * alpha;
    c8[(size_t)v * kBatch + col] = (1.0 - alpha) * rc;  // every in-edge e = (u -> v) deposits (c * w(e)) / W(u)
  }
}

// column -> list: every node of [0, n) that holds a contribution, with the prefix of the IN-degrees (k_wb_push locates
// an edge by it) and its contribution; the column is handed back all-zero.  *counter: 0 before, entries << 36 | edges after.
__global__ __launch_bounds__(256) void k_wbb_compact(uint32_t n, double* __restrict__ c8, uint32_t col,
                                                    const uint32_t* __restrict__ in_rp, int32_t* __restrict__ Fn,
                                                    uint32_t* __restrict__ eoffn, double* __restrict__ cF,
                                                    unsigned long long* counter) {
  const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
  const uint32_t lo = blockIdx.x * per;
  const uint32_t hi = lo + per < n ? lo + per : n;
  if (lo >= hi) return;
  block_range_compact(
      lo, hi, counter,
      [&](uint32_t v, unsigned long long* w) {
        if (!(c8[(size_t)v * kBatch + col] > 0.0)) return false;
        *w = in_rp[v + 1] - in_rp[v];
        return true;
      },
      [&](uint32_t v, uint32_t pos, unsigned long long eo, unsigned long long) {
        Fn[pos] = (int32_t)v;
        eoffn[pos] = (uint32_t)eo;
        cF[pos] = c8[(size_t)v * kBatch + col];
        c8[(size_t)v * kBatch + col] = 0.0;
      });
}

// The members of the scattered list that have no out-edges (a dead-end target, members of a set): k_wbb_apply rewrites
// the rows with out-edges only, so their entries would be gathered again two sweeps later.  Both arrays: zeros.
__global__ __launch_bounds__(256) void k_wbb_leave(const int32_t* __restrict__ F, uint32_t nf,
                                                  const unsigned long long* __restrict__ out_ext, double* __restrict__ c8a,
                                                  double* __restrict__ c8b, uint32_t col) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
    const int32_t v = F[i];
    if ((uint32_t)(out_ext[v] >> 32) != 0u) continue;
    c8a[(size_t)v * kBatch + col] = 0.0;
    c8b[(size_t)v * kBatch + col] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
int launch_wbb_scatter(pprhip_graph* S, const PushArgs& a, int fbuf, uint32_t nf) {
  const BatchState* bs = S->parent->batch;
  k_wbb_scatter<<<dim3(grid_for(nf, 256, 512)), dim3(256), 0, S->stream>>>(S->F[fbuf], nf, S->residue, S->reserve,
                                                                         bs->c8[bs->c8cur], (uint32_t)S->slot_index, a.alpha);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_wbb_compact(pprhip_graph* S, int out_fbuf, unsigned long long* d_counter) {
  const BatchState* bs = S->parent->batch;
  k_wbb_compact<<<dim3(grid_for(act_n(S), 1024, 1024)), dim3(256), 0, S->stream>>>(
      act_n(S), bs->c8[bs->c8cur], (uint32_t)S->slot_index, S->gr->in_rp, S->F[out_fbuf], S->eoff[out_fbuf], S->cF,
      d_counter);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_wbb_leave(pprhip_graph* S, int fbuf, uint32_t nf) {
  const BatchState* bs = S->parent->batch;
  if (!nf) return PPRHIP_OK;
  k_wbb_leave<<<dim3(grid_for(nf, 256, 512)), dim3(256), 0, S->stream>>>(S->F[fbuf], nf, S->gr->out_ext, bs->c8[0],
                                                                       bs->c8[1], (uint32_t)S->slot_index);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// One batched weighted backward sweep of the columns marked active in the batch state's staged slot arguments
// (h_slot_args): c8[c8cur] -> c8[c8cur ^ 1], every active column's new frontier counter into its slot's
// ctr->packed[out_slot] and into sweep_out.
int launch_wbb_sweep(pprhip_graph* P) {
  const GraphData* D = P->gr;
  BatchState* bs = P->batch;
  PPRHIP_CHECK_HIP(hipMemcpyAsync(bs->d_slot_args, bs->h_slot_args, sizeof(SlotArgs) * kBatch, hipMemcpyHostToDevice,
                                  P->stream));
  const uint32_t n_chunks = (uint32_t)((D->m + kChunkEdges - 1) / kChunkEdges);
  if (n_chunks) {
    constexpr uint32_t kWaves = 8;  // per workgroup of 512 threads
    const uint32_t want = (n_chunks + kWaves - 1) / kWaves;
    const uint32_t grid = std::min<uint32_t>(want, (uint32_t)D->n_cus * 4u);
    k_wbb_edges<<<dim3(grid), dim3(64 * kWaves), 0, P->stream>>>(
        D->out_ci, D->out_w, (unsigned long long)D->m, reinterpret_cast<const unsigned long long*>(D->start_flags_o),
        D->chunk_starts_o, n_chunks, bs->c8[bs->c8cur], bs->acc8);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  const uint32_t n_tiles = (D->n_nz_o + kWbbRows - 1) / kWbbRows;
  const uint32_t grid = std::min<uint32_t>(n_tiles, kApplyBlocks8);
  if (grid) {
    k_wbb_apply<<<dim3(grid), dim3(kWbbThreads), 0, P->stream>>>(D->nz_rows_o, D->n_nz_o, bs->acc8, D->in_rp, D->wsum,
                                                             bs->c8[bs->c8cur ^ 1], bs->d_slot_args, bs->blk_pack8,
                                                             kApplyBlocks8);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  k_wbb_reduce<<<dim3(kBatch), dim3(1024), 0, P->stream>>>(bs->blk_pack8, grid, kApplyBlocks8, bs->d_slot_args,
                                                         bs->sweep_out);
  PPRHIP_CHECK_HIP(hipGetLastError());
  bs->c8cur ^= 1;
  // what an unweighted backward sweep tells the forward sweeps' row history (launch_dense_level_b8): the arrays may hold
  // entries on rows without in-edges, so the next forward sweeps run over every tile
  bs->zin_full_left = 3;
  return PPRHIP_OK;
}

int init_kernels_weighted_bwd_batch() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_wbb_edges)));
  return PPRHIP_OK;
}

}  // namespace pprhip
