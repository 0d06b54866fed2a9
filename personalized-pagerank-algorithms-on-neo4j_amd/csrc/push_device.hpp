// push_device.hpp — what two or more of the level kernel files share (kernels_push.hip, kernels_dense.hip,
// kernels_dense_batch.hip, kernels_frontier.hip): device helpers first, launcher helpers behind them.  A helper that
// only one of them uses lives in that file.  For .hip files only.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "device_utils.hpp"
#include "engine.hpp"

namespace pprhip {

constexpr int kChunkEdges = 512;  // edges a wave of a dense sweep's edge kernel owns (k_dense_edges, k_dense_edges_b)

// A node that met the round's threshold at round start without being in the queue ("armed", see engine.hpp) is
// enqueued by the first push that reaches it (Forward_Push.java:226-231 tests the new residue only): whoever clears
// its bit appends it.
__device__ __forceinline__ bool take_armed(uint32_t* __restrict__ armed, int32_t u) {
  const uint32_t bit = 1u << ((uint32_t)u & 31u);
  if (!(armed[(uint32_t)u >> 5] & bit)) return false;
  return (atomicAnd(&armed[(uint32_t)u >> 5], ~bit) & bit) != 0;
}

// The dead-mass cell is read by every workgroup of a landing launch and zeroed by the last one to finish.
__device__ __forceinline__ void seed_land_done(unsigned int* done, DevCounters* ctr, int dead_slot) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(done, 1u) == gridDim.x - 1) {
      ctr->dead[dead_slot] = 0.0;
      *done = 0u;
    }
  }
}

// ---- launcher helpers
static inline uint32_t grid_for(uint64_t work, uint32_t per_block, uint32_t cap) {
  uint64_t b = (work + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (uint32_t)b;
}

// contribution buffer `cbuf` of a handle: its own array, or its column of the parent's c8 array
static inline CView cview(pprhip_graph* g, int cbuf) {
  if (g->parent) return CView{g->parent->batch->c8[cbuf], (uint32_t)kBatch, (uint32_t)g->slot_index};
  return CView{g->cdense[cbuf], 1u, 0u};
}

#define DISPATCH_MODE(MODEVAR, ...)                                       \
  switch (MODEVAR) {                                                      \
    case kFwdWhole: { constexpr int M = kFwdWhole; __VA_ARGS__; } break;  \
    case kFwdTopk: { constexpr int M = kFwdTopk; __VA_ARGS__; } break;    \
    case kBackward: { constexpr int M = kBackward; __VA_ARGS__; } break;  \
    default: { constexpr int M = kPower; __VA_ARGS__; } break;            \
  }

// The side of the graph a dense level sweeps: forward levels pull over the in-CSR, backward levels over the out-CSR.
// rp: the row pointers of the other side, along which a row that the level prepared pushes next.
struct SweepSide {
  const int32_t* ci;
  const uint8_t* start_flags;
  const uint32_t* chunk_starts;
  const int32_t *nz_rows, *z_rows;  // rows with / without edges on this side
  uint32_t n_nz, n_z;
  const unsigned long long* cross_bits;
  const uint32_t* rp;
};
static inline SweepSide sweep_side(const GraphData* D, bool backward) {
  if (backward)
    return {D->out_ci, D->start_flags_o, D->chunk_starts_o, D->nz_rows_o, D->z_rows_o, D->n_nz_o, D->n_z_o,
            D->cross_bits_o, D->in_rp};
  return {D->in_ci, D->start_flags, D->chunk_starts, D->nz_rows, D->zin_rows, D->n_nz, D->n_zin, D->cross_bits, D->out_rp};
}

// kernels_dense.hip: block partial counts -> ctr->packed[out_slot] (reuses the dense reducer with no dead mass)
int reduce_partials(pprhip_graph* g, uint32_t n_blocks, int out_slot, int dead_slot, bool with_dead);

}  // namespace pprhip
