// kernels_compact.hip — sparse results: a result vector as its (id, value) entries over a threshold, compacted on the
// device in original-id order (DESIGN.md §2 "Sparse results").
//
// The compaction runs over the ORIGINAL-id space and is fused with the permutation copy_out pays for a dense fetch:
// the thread of id v reads x[old2new[v]] (x[v] on a handle that keeps the caller's ids), tests it against the threshold,
// and a kept entry gets the position "kept entries of smaller id" - an ORDERED compaction, unlike the ballot / atomic
// idiom of k_sweep_support, so by-id needs no sort and every run writes the same bytes.  No n-sized intermediate:
//   k_entries_count    kept entries per TILE of kCompactTile ids (wave ballots, popcounts, one sum per workgroup)
//   (rocPRIM)          exclusive scan of the tile counts: a tile's first output position, the total behind the last
//   k_entries_offsets  the scan at every vector's first tile: the CSR offsets of a store, {0, total} of one vector
//   k_entries_scatter  the same ballots again; position = base[tile] + kept in the turns and waves before + kept in
//                      the lanes below.  Tiles without an entry leave at once: a small support reads the vector once.
//   (rocPRIM)          by value: stable descending radix sort on the value bits (positive doubles order like their
//                      bits; ties keep the id order they came in), for a store a second stable sort by vector
//   k_entries_unpack   ... and the ids out of the words that rode along
// A second grid dimension runs over the vectors of a store; tiles are numbered vector-major, so one scan serves all.
// Three launches with the host's one wait for the total between scan and scatter (the buffers are sized by it), not a
// single-pass look-back: that one would have to own n entries of output per vector before it knows the count.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "device_utils.hpp"
#include "engine.hpp"

namespace pprhip {

typedef unsigned long long u64;

constexpr uint32_t kCompactRowsPerLaunch = 32768;  // vectors per launch (the grid's second dimension)

// the ids of tile `tile`, turn k: tile * kCompactTile + k * 256 + thread - consecutive lanes, consecutive ids
__device__ __forceinline__ bool compact_take(const double* __restrict__ x, const int32_t* __restrict__ old2new,
                                             uint32_t n, uint64_t v, double threshold, double* xv_out) {
  if (v >= n) return false;
  const double xv = x[old2new ? (uint32_t)old2new[v] : (uint32_t)v];
  *xv_out = xv;
  return xv > threshold;  // (false for NaN and for -0.0 at threshold 0)
}

__global__ __launch_bounds__(256) void k_entries_count(const double* __restrict__ x, const int32_t* __restrict__ old2new,
                                                        uint32_t n, uint32_t tiles, uint32_t row0, double threshold,
                                                        u64* __restrict__ cnt) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t row = row0 + blockIdx.y;
  const double* xr = x + (size_t)row * n;
  const uint64_t v0 = (uint64_t)blockIdx.x * kCompactTile + threadIdx.x;
  uint32_t c = 0;
#pragma unroll
  for (uint32_t k = 0; k < kCompactPer; ++k) {
    double xv;
    const bool take = compact_take(xr, old2new, n, v0 + k * 256u, threshold, &xv);
    c += (uint32_t)__popcll(__ballot(take));
  }
  if (lane_id() == 0) s_cnt[wave_id()] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[(size_t)row * tiles + blockIdx.x] = (u64)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(256) void k_entries_offsets(const u64* __restrict__ base, uint32_t tiles, uint32_t rows,
                                                          u64* __restrict__ offs) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i <= rows; i += gridDim.x * 256u) offs[i] = base[(size_t)i * tiles];
}

template <bool PACKED>
__global__ __launch_bounds__(256) void k_entries_scatter(const double* __restrict__ x,
                                                          const int32_t* __restrict__ old2new, uint32_t n,
                                                          uint32_t tiles, uint32_t row0, double threshold,
                                                          const u64* __restrict__ base, u64* __restrict__ val,
                                                          uint32_t* __restrict__ id, u64* __restrict__ pk) {
  __shared__ uint32_t s_cnt[kCompactPer][4];
  const uint32_t row = row0 + blockIdx.y;
  const size_t t = (size_t)row * tiles + blockIdx.x;
  const u64 b0 = base[t];
  if (base[t + 1] == b0) return;  // nothing kept here (the same for the whole workgroup)
  const double* xr = x + (size_t)row * n;
  const uint64_t v0 = (uint64_t)blockIdx.x * kCompactTile + threadIdx.x;
  const int lane = lane_id(), wave = wave_id();
  double xv[kCompactPer];
  u64 mask[kCompactPer];
#pragma unroll
  for (uint32_t k = 0; k < kCompactPer; ++k) {
    xv[k] = 0.0;
    mask[k] = __ballot(compact_take(xr, old2new, n, v0 + k * 256u, threshold, &xv[k]));
    if (lane == 0) s_cnt[k][wave] = (uint32_t)__popcll(mask[k]);
  }
  __syncthreads();
  uint32_t before = 0;  // kept in the turns before turn k, and in turn k's waves before this one
#pragma unroll
  for (uint32_t k = 0; k < kCompactPer; ++k) {
    uint32_t mine = before;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) mine += s_cnt[k][w];
      before += s_cnt[k][w];
    }
    if ((mask[k] >> lane) & 1ull) {
      // (< base[t + 1] <= the total the buffers were sized for: the count kernel ran the same test on the same vector)
      const u64 pos = b0 + mine + (u64)__popcll(mask[k] & ((1ull << lane) - 1ull));
      val[pos] = (u64)__double_as_longlong(xv[k]);
      const uint32_t v = (uint32_t)(v0 + k * 256u);
      if (PACKED) pk[pos] = (u64)row << 32 | v;
      else id[pos] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_entries_unpack(const u64* __restrict__ pk, u64 count, uint32_t* __restrict__ id) {
  for (u64 i = blockIdx.x * 256ull + threadIdx.x; i < count; i += (u64)gridDim.x * 256ull) id[i] = (uint32_t)pk[i];
}

// ------------------------------------------------------------------ launchers
// the library calls' scratch: grown when a call asks for more than there is
static int compact_tmp(SparseWs* w, size_t need) {
  if (need <= w->tmp_bytes) return PPRHIP_OK;
  if (w->tmp) (void)hipFree(w->tmp);  // (waits for the work queued on it)
  w->tmp = nullptr;
  w->tmp_bytes = 0;
  const hipError_t e = hipMalloc(&w->tmp, need);
  if (e != hipSuccess) {
    set_error("sparse results: hipMalloc(%zu bytes) failed: %s", need, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? PPRHIP_ERR_OOM : PPRHIP_ERR_HIP;
  }
  w->tmp_bytes = need;
  return PPRHIP_OK;
}

static uint32_t compact_tiles(const pprhip_graph* g) { return (g->gr->n + kCompactTile - 1u) / kCompactTile; }

int launch_compact_count(pprhip_graph* g, SparseWs* w, const double* x, uint32_t rows, double threshold) {
  const GraphData* D = g->gr;
  const uint32_t tiles = compact_tiles(g);
  const size_t T = (size_t)rows * tiles;  // (<= w->tile_cap, rows + 1 <= w->offs_cap: sparse.cpp)
  const int32_t* o2n = D->relabeled ? D->old2new : nullptr;
  PPRHIP_CHECK_HIP(hipMemsetAsync(w->cnt + T, 0, sizeof(u64), g->stream));
  for (uint32_t r0 = 0; r0 < rows; r0 += kCompactRowsPerLaunch) {
    const uint32_t nr = std::min(rows - r0, kCompactRowsPerLaunch);
    hipLaunchKernelGGL(k_entries_count, dim3(tiles, nr), dim3(256), 0, g->stream, x, o2n, D->n, tiles, r0, threshold, w->cnt);
  }
  PPRHIP_CHECK_HIP(hipGetLastError());
  size_t b = 0;
  if (rocprim::exclusive_scan(nullptr, b, w->cnt, w->base, 0ull, T + 1, rocprim::plus<u64>(), g->stream) != hipSuccess) {
    set_error("sparse results: sizing the device scan failed");
    return PPRHIP_ERR_HIP;
  }
  PPRHIP_TRY(compact_tmp(w, std::max<size_t>(b, 16)));
  b = w->tmp_bytes;
  if (rocprim::exclusive_scan(w->tmp, b, w->cnt, w->base, 0ull, T + 1, rocprim::plus<u64>(), g->stream) != hipSuccess) {
    set_error("sparse results: the device scan failed");
    return PPRHIP_ERR_HIP;
  }
  const uint32_t grid = std::min<uint32_t>((rows + 1u + 255u) / 256u, 1024u);
  hipLaunchKernelGGL(k_entries_offsets, dim3(grid), dim3(256), 0, g->stream, w->base, tiles, rows, w->offs);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int launch_compact_scatter(pprhip_graph* g, SparseWs* w, const double* x, uint32_t rows, double threshold, bool packed) {
  const GraphData* D = g->gr;
  const uint32_t tiles = compact_tiles(g);
  const int32_t* o2n = D->relabeled ? D->old2new : nullptr;
  for (uint32_t r0 = 0; r0 < rows; r0 += kCompactRowsPerLaunch) {
    const uint32_t nr = std::min(rows - r0, kCompactRowsPerLaunch);
    if (packed)
      hipLaunchKernelGGL(k_entries_scatter<true>, dim3(tiles, nr), dim3(256), 0, g->stream, x, o2n, D->n, tiles, r0, threshold,
                         w->base, w->val[0], w->id, w->pk[0]);
    else
      hipLaunchKernelGGL(k_entries_scatter<false>, dim3(tiles, nr), dim3(256), 0, g->stream, x, o2n, D->n, tiles, r0,
                         threshold, w->base, w->val[0], w->id, w->pk[0]);
  }
  PPRHIP_CHECK_HIP(hipGetLastError());
  w->val_out = w->val[0];
  return PPRHIP_OK;
}

// Stable sorts, least significant criterion first: the entries arrive in (vector, id) order; by value bits descending,
// then (a store) by vector ascending.  Kept values are positive doubles: bit 63 is clear in every key.
int launch_compact_sort(pprhip_graph* g, SparseWs* w, uint64_t total, uint32_t rows) {
  unsigned row_bits = 0;
  while (row_bits < 32 && (1ull << row_bits) < (u64)rows) ++row_bits;
  rocprim::double_buffer<u64> dv(w->val[0], w->val[1]);
  rocprim::double_buffer<u64> dp(w->pk[0], w->pk[1]);
  size_t b0 = 0, b1 = 0;
  if (rocprim::radix_sort_pairs_desc(nullptr, b0, dv, dp, (size_t)total, 0u, 63u, g->stream) != hipSuccess ||
      (row_bits && rocprim::radix_sort_pairs(nullptr, b1, dp, dv, (size_t)total, 32u, 32u + row_bits, g->stream) != hipSuccess)) {
    set_error("sparse results: sizing the device sort failed");
    return PPRHIP_ERR_HIP;
  }
  PPRHIP_TRY(compact_tmp(w, std::max<size_t>(std::max(b0, b1), 16)));
  size_t b = w->tmp_bytes;
  if (rocprim::radix_sort_pairs_desc(w->tmp, b, dv, dp, (size_t)total, 0u, 63u, g->stream) != hipSuccess) {
    set_error("sparse results: the device sort by value failed");
    return PPRHIP_ERR_HIP;
  }
  b = w->tmp_bytes;
  if (row_bits && rocprim::radix_sort_pairs(w->tmp, b, dp, dv, (size_t)total, 32u, 32u + row_bits, g->stream) != hipSuccess) {
    set_error("sparse results: the device sort by vector failed");
    return PPRHIP_ERR_HIP;
  }
  const uint32_t grid = (uint32_t)std::min<uint64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_entries_unpack, dim3(grid), dim3(256), 0, g->stream, dp.current(), (u64)total, w->id);
  PPRHIP_CHECK_HIP(hipGetLastError());
  w->val_out = dv.current();
  return PPRHIP_OK;
}

int init_kernels_compact() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_entries_count)));
  return PPRHIP_OK;
}

}  // namespace pprhip
