// kernels_weighted_bwd.hip — the backward direction over weighted relationships for gfx950 (MI355X): the levels of a
// weighted backward push, the weighted survival iteration and the walks of a weighted pair (DESIGN.md §2 "Weighted
// backward direction"; weighted_bwd.cpp drives them).  Popping v with residue r credits reserve(v) += alpha r and sends
// c(v) = (1 - alpha) r back along every in-edge e = (u -> v): r(u) += (c(v) * w(e)) / W(u).  The mirror image of
// kernels_weighted.hip, with which it shares weighted_device.hpp; the unweighted kernels carry no weight branch.
//
//   sparse  k_wb_prepare (per frontier node: take the residue, credit the reserve, c = (1 - alpha) r) then k_wb_push:
//           edge-parallel over the frontier's in-rows (entries staged in LDS, an edge finds its entry by binary search
//           over the staged edge offsets, so a hub target's row is spread over lanes), streams in_ci / in_w, gathers
//           W(u), one returning fp64 atomic per edge; crossings of the backward test (!(old > rmax) && new > rmax,
//           strict, no degree in it) are collected in LDS and appended with one packed atomic per tile, carrying the
//           IN-degree, along which the node pushes next.
//   dense   k_wb_edges: k_w_dense_edges' flat pull sweep over out_ci / out_w - a wave owns 512 consecutive out-edges,
//           gathers x[dst], multiplies by the weight, sums by out-row with the segmented wave scan into acc_nz.
//           k_wb_dense_apply divides the row sum by W(u) once, lands it, tests and prepares crossing rows.
//   survival  the same edge kernel with x = S_old, then k_wb_surv_apply: S' = alpha + (1 - alpha) * rowsum / W(u).
//           A row is summed by however many waves its edges span, so hub rows need no path of their own.
//   pairs   k_wb_pair_walk: k_pair_walk's work items and refill order with the weighted walker step.
//
// All arithmetic is IEEE double with -ffp-contract=off (tests/weighted_bwd_ref.py restates the rules).
#include "weighted_device.hpp"

namespace pprhip {

// ------------------------------------------------------------------------------------------------
// sparse level, step 1: every frontier node gives up its residue
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_wb_prepare(const int32_t* __restrict__ F, uint32_t nf, double* __restrict__ res,
                                                     double* __restrict__ reserve, double* __restrict__ cF,
                                                     double* __restrict__ c_dense, unsigned long long* next_counter,
                                                     double alpha) {
  if (next_counter && blockIdx.x == 0 && threadIdx.x == 0) *next_counter = 0ull;  // the list k_wb_push appends to
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
    const int32_t v = F[i];
    const double rc = res[v];
    res[v] = 0.0;
    reserve[v] = reserve[v] + rc * alpha;
    const double c = (1.0 - alpha) * rc;  // every in-edge e = (u -> v) deposits (c * w(e)) / W(u)
    if (c_dense)
      c_dense[v] = c;
    else
      cF[i] = c;
  }
}

// ------------------------------------------------------------------------------------------------
// sparse level, step 2: contributions land edge by edge on the sources of the frontier's in-edges
// ------------------------------------------------------------------------------------------------
// the backward test of the engine (push_finish<kBackward>): strict, un-normalised; the in-degree is only read for a
// node that crosses
__device__ __forceinline__ void wb_push_finish(int32_t u, double add, double old, const uint32_t* __restrict__ in_rp,
                                               WNewList* nl, double rmax) {
  const double nw = old + add;
  if (!(old > rmax) && nw > rmax) {
    const uint32_t slot = atomicAdd(&nl->count, 1u);
    nl->node[slot] = u;
    nl->deg[slot] = in_rp[u + 1] - in_rp[u];
  }
}

__global__ __launch_bounds__(256) void k_wb_push(const int32_t* __restrict__ F, const double* __restrict__ cF,
                                                  const uint32_t* __restrict__ eoff, uint32_t nf, unsigned long long E,
                                                  const uint32_t* __restrict__ in_rp, const int32_t* __restrict__ in_ci,
                                                  const double* __restrict__ in_w, const double* __restrict__ wsum,
                                                  double* __restrict__ res, int32_t* __restrict__ Fn,
                                                  uint32_t* __restrict__ eoffn, unsigned long long* out_counter,
                                                  double rmax) {
  __shared__ uint32_t s_eoff[kWStage + 1];
  __shared__ uint32_t s_row[kWStage];
  __shared__ double s_c[kWStage];
  __shared__ uint32_t s_i0;
  __shared__ WNewList s_new;
  const int tid = threadIdx.x;
  if (tid == 0) s_new.count = 0;
  __syncthreads();

  const unsigned long long n_tiles = (E + kWTile - 1) / kWTile;
  for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const unsigned long long tile_lo = t * kWTile;
    const unsigned long long tile_hi = (tile_lo + kWTile < E) ? tile_lo + kWTile : E;
    if (tid == 0) {  // last frontier index whose edge range starts at or before tile_lo
      uint32_t lo = 0, hi = nf;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((unsigned long long)eoff[mid] <= tile_lo) lo = mid + 1; else hi = mid;
      }
      s_i0 = lo - 1;
    }
    __syncthreads();
    uint32_t ci0 = s_i0;
    unsigned long long ce = tile_lo;
    while (ce < tile_hi) {
      const uint32_t cnt = (nf - ci0 < (uint32_t)kWStage) ? nf - ci0 : (uint32_t)kWStage;
      if (cnt == 0) break;
      for (uint32_t j = tid; j <= cnt; j += 256) {
        const uint32_t idx = ci0 + j;
        s_eoff[j] = idx < nf ? eoff[idx] : (uint32_t)E;
        if (j < cnt) {
          s_row[j] = in_rp[F[idx]];  // first in-edge of the entry's row
          s_c[j] = cF[idx];
        }
      }
      __syncthreads();
      const unsigned long long cov_hi = ((unsigned long long)s_eoff[cnt] < tile_hi) ? s_eoff[cnt] : tile_hi;
      // four edges per thread in flight: col_idx and weight loads, then the W gathers, then atomics, then tests
      for (unsigned long long base = ce + tid; base < cov_hi; base += 1024) {
        int32_t u[4];
        double cw[4], add[4], old[4];
        bool valid[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned long long e = base + 256ull * q;
          valid[q] = e < cov_hi;
          u[q] = 0;
          cw[q] = 0.0;
          if (valid[q]) {
            const uint32_t e32 = (uint32_t)e;
            uint32_t lo = 0, hi = cnt;  // last staged entry whose range starts at or before e
            while (lo < hi) {
              const uint32_t mid = (lo + hi) >> 1;
              if (s_eoff[mid] <= e32) lo = mid + 1; else hi = mid;
            }
            const uint32_t j = lo - 1;
            const uint32_t pos = s_row[j] + (e32 - s_eoff[j]);
            u[q] = in_ci[pos];
            cw[q] = s_c[j] * in_w[pos];
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) add[q] = valid[q] ? cw[q] / wsum[u[q]] : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          old[q] = 0.0;
          if (valid[q]) old[q] = atomic_add_ret(&res[u[q]], add[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (valid[q]) wb_push_finish(u[q], add[q], old[q], in_rp, &s_new, rmax);
      }
      __syncthreads();
      ce = cov_hi;
      ci0 += cnt;
    }
    w_flush_new(&s_new, Fn, eoffn, out_counter);
  }
}

// ------------------------------------------------------------------------------------------------
// dense level and survival iteration: flat pull sweep over out_ci / out_w
// ------------------------------------------------------------------------------------------------
// out_ci is padded to whole chunks like in_ci (index 0, no row-start flag); out_w holds exactly m weights, so the lanes
// of the last chunk that reach beyond m read their weights one by one, 0.0 for a padding edge.
__device__ __forceinline__ WChunkRegs wb_load_chunk(const int32_t* __restrict__ out_ci, const double* __restrict__ out_w,
                                                    unsigned long long m, const uint8_t* __restrict__ start_flags,
                                                    uint32_t c, int lane) {
  const unsigned long long e0 = (unsigned long long)c * kChunkEdges + 8ull * lane;
  if (e0 + 8ull <= m) return w_load_chunk(out_ci, out_w, start_flags, c, lane);
  typedef int v4i __attribute__((ext_vector_type(4)));
  const v4i* q = reinterpret_cast<const v4i*>(out_ci + e0);
  const v4i x = __builtin_nontemporal_load(q), y = __builtin_nontemporal_load(q + 1);
  WChunkRegs r;
  r.ia = make_int4(x.x, x.y, x.z, x.w);
  r.ib = make_int4(y.x, y.y, y.z, y.w);
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = e0 + i < m ? out_w[e0 + i] : 0.0;
  r.fb = start_flags[e0 >> 3];
  return r;
}

// One wave per chunk of 512 consecutive out-edges: acc_nz[row ordinal] = sum over the row's edges e = (u -> v) of
// x[v] * w(e) (k_w_dense_edges over the other CSR).  Rows that start and end inside the wave are stored, the (at most
// two) rows that cross the chunk boundary use an fp64 atomic on acc_nz, which the apply kernels leave zero.
__global__ __launch_bounds__(512) void k_wb_edges(const int32_t* __restrict__ out_ci, const double* __restrict__ out_w,
                                                   unsigned long long m, const uint8_t* __restrict__ start_flags,
                                                   const uint32_t* __restrict__ chunk_starts, uint32_t n_chunks,
                                                   const double* __restrict__ x, double* __restrict__ acc_nz) {
  const int lane = lane_id();
  const uint32_t waves_per_block = blockDim.x >> 6;
  const uint32_t stride = gridDim.x * waves_per_block;
  uint32_t c = blockIdx.x * waves_per_block + (uint32_t)__builtin_amdgcn_readfirstlane(wave_id());
  if (c >= n_chunks) return;
  WChunkRegs cur = wb_load_chunk(out_ci, out_w, m, start_flags, c, lane);
  for (; c < n_chunks; c += stride) {
    // the next chunk's streams are requested before this chunk's gathers, so their latency is hidden
    WChunkRegs nxt = cur;
    if (c + stride < n_chunks) nxt = wb_load_chunk(out_ci, out_w, m, start_flags, c + stride, lane);
    const uint32_t cs = chunk_starts[c];
    const uint32_t fb = cur.fb;
    const int32_t idx[8] = {cur.ia.x, cur.ia.y, cur.ia.z, cur.ia.w, cur.ib.x, cur.ib.y, cur.ib.z, cur.ib.w};
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = x[idx[i]];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = v[i] * cur.w[i];
    // row index of a segment = (row starts at or before its first edge) - 1
    const uint32_t pc = __popc(fb);
    const uint32_t incl = wave_incl_scan_u32_dpp(pc);
    const uint32_t before = cs + incl - pc;  // row starts before this lane's first edge
    double seg = 0.0, first_seg = 0.0;
    uint32_t k = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if ((fb >> i) & 1u) {
        if (k == 0)
          first_seg = seg;  // closes the row carried in from earlier lanes
        else
          acc_nz[before + k - 1] = seg;  // a row that starts and ends inside this lane
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
        if (started_here)
          acc_nz[before - 1] = tot;
        else
          atomic_add_noret(&acc_nz[before - 1], tot);  // began in an earlier chunk
      }
    }
    if (lane == 63) {  // the row still open at the end of the chunk
      const uint32_t starts = cs + incl;
      if (starts > 0 && sval != 0.0) atomic_add_noret(&acc_nz[starts - 1], sval);
    }
    cur = nxt;
  }
}

// One thread per row with out-edges: divides the row sum by W(u) once, lands it, tests the backward threshold and
// prepares a crossing row for the next level in place (k_w_dense_apply, mirrored: no dead-end mass, no source row).
__global__ __launch_bounds__(256) void k_wb_dense_apply(const int32_t* __restrict__ nz_rows, uint32_t n_nz,
                                                         double* __restrict__ acc_nz, const uint32_t* __restrict__ in_rp,
                                                         const double* __restrict__ wsum, double* __restrict__ c_next,
                                                         double* __restrict__ res, double* __restrict__ reserve,
                                                         unsigned long long* __restrict__ blk_pack, double alpha,
                                                         double rmax) {
  __shared__ unsigned long long s_red2[4];
  const int tid = threadIdx.x;
  const uint32_t j = blockIdx.x * 256u + tid;
  unsigned long long pack = 0;
  if (j < n_nz) {
    const int32_t u = nz_rows[j];
    const double acc = acc_nz[j];
    acc_nz[j] = 0.0;
    double cn = 0.0;
    if (acc > 0.0) {
      const double add = acc / wsum[u];
      const double old = res[u];
      const double nw = old + add;
      if (!(old > rmax) && nw > rmax) {  // becomes a frontier node of the next level: prepare it right here
        reserve[u] = reserve[u] + nw * alpha;
        if (old != 0.0) res[u] = 0.0;
        cn = (1.0 - alpha) * nw;
        pack = (1ull << kPackShift) | (unsigned long long)(in_rp[u + 1] - in_rp[u]);
      } else {
        res[u] = nw;
      }
    }
    c_next[u] = cn;
  }
  const unsigned long long ps = block_sum_u64(pack, s_red2);  // per-workgroup partials; k_dense_reduce sums them
  if (tid == 0) blk_pack[blockIdx.x] = ps;
}

// max over the workgroup of non-negative doubles as bit patterns, one atomicMax per workgroup (kernels_walk.hip:
// surv_max_out)
__device__ __forceinline__ void wb_max_out(unsigned long long mx, unsigned long long* __restrict__ dmax) {
  __shared__ unsigned long long s_max[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_down(mx, o);
    mx = y > mx ? y : mx;
  }
  if (lane_id() == 0) s_max[wave_id()] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) mx = s_max[w] > mx ? s_max[w] : mx;
    if (mx) atomicMax(dmax, mx);
  }
}

// S'(u) = alpha + (1 - alpha) * rowsum / W(u) for the rows with out-edges; a dead end keeps alpha, which both buffers
// hold from the start.  dmax != nullptr: max |S' - S| goes to *dmax.
__global__ __launch_bounds__(256) void k_wb_surv_apply(const int32_t* __restrict__ nz_rows, uint32_t n_nz,
                                                        double* __restrict__ acc_nz, const double* __restrict__ wsum,
                                                        const double* __restrict__ s_old, double* __restrict__ s_new,
                                                        double alpha, unsigned long long* __restrict__ dmax) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  unsigned long long mx = 0ull;
  if (j < n_nz) {
    const int32_t u = nz_rows[j];
    const double acc = acc_nz[j];
    acc_nz[j] = 0.0;
    const double s = alpha + (1.0 - alpha) * acc / wsum[u];
    s_new[u] = s;
    if (dmax) {
      const double dx = fabs(s - s_old[u]);
      __builtin_memcpy(&mx, &dx, 8);
    }
  }
  if (dmax) wb_max_out(mx, dmax);
}

// ------------------------------------------------------------------------------------------------
// weighted pairs: the gather walks of one target's sources
// ------------------------------------------------------------------------------------------------
// k_pair_walk with the weighted walker: work item (p, c) = the walks [c * chunk_walks, min(w, (c + 1) * chunk_walks))
// of pair p, one wave per item; the walks are pprhip_weighted_random_walk_batch's at stream PPRHIP_PAIR_WALK_STREAM,
// no zero-hop skip.  A lane whose walk has stopped adds residue[terminal] to its register and takes the item's next
// walk in ballot order; the wave's sum goes to part[p * chunks + c]: no atomics on a pair's value.
__global__ __launch_bounds__(64) void k_wb_pair_walk(const int32_t* __restrict__ src, uint32_t n_pairs, uint32_t chunks,
                                                      unsigned long long chunk_walks, unsigned long long walks,
                                                      WWalkGraph G, const int32_t* __restrict__ new2old,
                                                      const double* __restrict__ residue, double alpha, uint32_t k0,
                                                      uint32_t k1, double* __restrict__ part,
                                                      unsigned long long* __restrict__ steps_out) {
  const int lane = threadIdx.x;
  const unsigned long long items = (unsigned long long)n_pairs * chunks;
  unsigned long long steps = 0;
  for (unsigned long long it = blockIdx.x; it < items; it += gridDim.x) {
    const uint32_t p = (uint32_t)(it / chunks), c = (uint32_t)(it % chunks);
    const int32_t s = src[p];
    const unsigned long long sext = G.out_ext[s];
    const int32_t s_orig = new2old[s];
    const unsigned long long lo = (unsigned long long)c * chunk_walks;
    const unsigned long long hi = lo + chunk_walks < walks ? lo + chunk_walks : walks;
    unsigned long long cursor = lo;
    double acc = 0.0;
    WWalker w;
    bool walking = false;
    for (;;) {
      const unsigned long long need = __ballot(!walking);
      if (need && cursor < hi) {
        const unsigned long long avail = hi - cursor;
        const uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
        if (!walking && rank < avail) {
          w_walker_init(w, s, sext, s_orig, cursor + rank, PPRHIP_PAIR_WALK_STREAM, false);
          if ((sext >> 32) == 0) acc += residue[s];  // a dead-end start is its own terminal
          else walking = true;
        }
        const unsigned long long want = __popcll(need);
        cursor += want < avail ? want : avail;
      }
      if (__ballot(walking) == 0) {
        if (cursor >= hi) break;
        continue;
      }
      if (walking && w_walker_step(w, G, alpha, k0, k1)) {
        acc += residue[w.cur];
        steps += w.moves;
        walking = false;
      }
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) part[(size_t)p * chunks + c] = acc;
  }
  steps = wave_sum_u64(steps);
  if (lane == 0 && steps) atomic_add_u64(steps_out, steps);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
int launch_wb_prepare(pprhip_graph* g, const PushArgs& a, int fbuf, uint32_t nf, bool scatter_dense, int cbuf,
                      unsigned long long* next_counter) {
  const uint32_t grid = grid_for(nf, 256, 512);
  k_wb_prepare<<<dim3(grid), dim3(256), 0, g->stream>>>(g->F[fbuf], nf, g->residue, g->reserve, g->cF,
                                                        scatter_dense ? g->cdense[cbuf] : nullptr, next_counter, a.alpha);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_wb_push(pprhip_graph* g, const PushArgs& a, int fbuf, uint32_t nf, uint64_t ef,
                   unsigned long long* next_counter) {
  if (nf == 0 || ef == 0) return PPRHIP_OK;
  const uint32_t grid = grid_for(ef, kWTile, 2048);
  k_wb_push<<<dim3(grid), dim3(256), 0, g->stream>>>(g->F[fbuf], g->cF, g->eoff[fbuf], nf, (unsigned long long)ef,
                                                     g->gr->in_rp, g->gr->in_ci, g->gr->in_w, g->gr->wsum, g->residue,
                                                     g->F[fbuf ^ 1], g->eoff[fbuf ^ 1], next_counter, a.rmax);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// the edge sweep both dense forms share: acc_nz[out-row ordinal] = sum of x[dst] * w over the row
static int launch_wb_edges(pprhip_graph* g, const double* x) {
  const GraphData* D = g->gr;
  const uint32_t n_chunks = (uint32_t)((D->m + kChunkEdges - 1) / kChunkEdges);
  if (!n_chunks) return PPRHIP_OK;
  constexpr uint32_t kWaves = 8;  // per workgroup of 512 threads
  const uint32_t want = (n_chunks + kWaves - 1) / kWaves;
  const uint32_t grid = std::min<uint32_t>(want, (uint32_t)D->n_cus * 4u);
  k_wb_edges<<<dim3(grid), dim3(64 * kWaves), 0, g->stream>>>(D->out_ci, D->out_w, (unsigned long long)D->m,
                                                             D->start_flags_o, D->chunk_starts_o, n_chunks, x, g->acc_nz);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_wb_dense_level(pprhip_graph* g, const PushArgs& a, int cbuf, int out_slot) {
  const GraphData* D = g->gr;
  PPRHIP_TRY(launch_wb_edges(g, g->cdense[cbuf]));
  const uint32_t grid = (D->n_nz_o + 255) / 256;
  if (grid) {
    k_wb_dense_apply<<<dim3(grid), dim3(256), 0, g->stream>>>(D->nz_rows_o, D->n_nz_o, g->acc_nz, D->in_rp, D->wsum,
                                                              g->cdense[cbuf ^ 1], g->residue, g->reserve, g->blk_pack,
                                                              a.alpha, a.rmax);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  return reduce_partials(g, grid, out_slot, 0, false);
}

int launch_wb_survival_iter(pprhip_graph* g, const double* s_old, double* s_new, double alpha, unsigned long long* dmax) {
  const GraphData* D = g->gr;
  PPRHIP_TRY(launch_wb_edges(g, s_old));
  const uint32_t grid = (D->n_nz_o + 255) / 256;
  if (grid) {
    k_wb_surv_apply<<<dim3(grid), dim3(256), 0, g->stream>>>(D->nz_rows_o, D->n_nz_o, g->acc_nz, D->wsum, s_old, s_new,
                                                             alpha, dmax);
    PPRHIP_CHECK_HIP(hipGetLastError());
  }
  return PPRHIP_OK;
}

int launch_wb_pair_walk(pprhip_graph* g, const int32_t* d_src, uint32_t n_pairs, uint32_t chunks, uint64_t chunk_walks,
                        uint64_t walks, double alpha, uint64_t seed, double* d_part, unsigned long long* d_steps) {
  const uint64_t items = (uint64_t)n_pairs * chunks;
  if (items == 0) return PPRHIP_OK;
  const uint64_t cap = (uint64_t)g->gr->n_cus * 16u;
  const uint32_t grid = (uint32_t)(items < cap ? items : cap);
  const WWalkGraph G{g->gr->out_ext, g->gr->out_ci, g->gr->out_cum, g->gr->wsum};
  k_wb_pair_walk<<<dim3(grid), dim3(64), 0, g->stream>>>(d_src, n_pairs, chunks, (unsigned long long)chunk_walks,
                                                         (unsigned long long)walks, G, g->gr->new2old, g->residue, alpha,
                                                         (uint32_t)seed, (uint32_t)(seed >> 32), d_part, d_steps);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int init_kernels_weighted_bwd() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_wb_push)));
  return PPRHIP_OK;
}

}  // namespace pprhip
