// kernels_target.hip — single-target queries (include/pprhip.h "single targets", DESIGN.md §2 "Single targets") for
// gfx950: the start of a backward push from a weighted target set, and the pass that turns the finished push's
// reserve p (the leaking PPR's lower bound) into the engine's restarting PPR, value(s) = p(s) / S(s).  The levels in
// between are the backward kernels of kernels_push.hip and kernels_dense_batch.hip unchanged: sharing their batched
// sweeps is the point.
#include <algorithm>

#include "device_utils.hpp"
#include "engine.hpp"

namespace pprhip {

constexpr int kTargetItems = 8;  // consecutive members / nodes per thread: 16-byte loads, one tile = 2048

// Start of a target set: r = w on the members (ids distinct, internal; the table is padded to whole groups of eight, so
// a thread's ids are two 16-byte loads and its weights four).  A member with in-edges whose weight passes the backward
// push's enqueue test (push_finish<kBackward>: r > rmax, strict and un-normalised) goes on the first frontier list with
// its in-degree as edge weight - one packed atomic per tile of 2048 members (block_tile_compact) - the others keep
// their weight as residue, which a later push may lift over the threshold like any other residue.  A member without
// in-edges has nobody to push to: popping it would move alpha * w to its reserve and drop the rest, whatever the
// threshold, so that is done here (the single target's p(t) = alpha).  Backward levels neither arm nor park: flags and
// armed bits stay as they are, as behind seed_single.  counter: zero at launch.  The trip count is uniform per
// workgroup (whole tiles), so the barriers of the compaction are met by every wave, tail waves included.
__global__ __launch_bounds__(256) void k_target_init(const int32_t* __restrict__ id, const double* __restrict__ w,
                                                      uint32_t count, const uint32_t* __restrict__ in_rp,
                                                      double* __restrict__ res, double* __restrict__ reserve,
                                                      int32_t* __restrict__ F, uint32_t* __restrict__ eoff,
                                                      unsigned long long* counter, double alpha, double rmax) {
  const uint32_t tile = 256u * kTargetItems;
  const uint32_t n_tiles = (count + tile - 1) / tile;
  for (uint32_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const uint32_t i0 = tl * tile + threadIdx.x * kTargetItems;
    int32_t u[kTargetItems];
    double x[kTargetItems];
    bool take[kTargetItems];
    unsigned long long deg[kTargetItems];
    if (i0 < count) {  // (padding: the whole group exists)
      const int4* p4 = reinterpret_cast<const int4*>(id + i0);
      const int4 a = p4[0], b = p4[1];
      u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w;
      u[4] = b.x; u[5] = b.y; u[6] = b.z; u[7] = b.w;
      const double2* w2 = reinterpret_cast<const double2*>(w + i0);
#pragma unroll
      for (int i = 0; i < kTargetItems / 2; ++i) {
        const double2 v = w2[i];
        x[2 * i] = v.x;
        x[2 * i + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int i = 0; i < kTargetItems; ++i) {
        u[i] = 0;
        x[i] = 0.0;
      }
    }
#pragma unroll
    for (int i = 0; i < kTargetItems; ++i) {
      take[i] = false;
      deg[i] = 0;
      if (i0 + i < count) {
        const uint32_t d = in_rp[u[i] + 1] - in_rp[u[i]];
        if (d == 0) {
          reserve[u[i]] = x[i] * alpha;
        } else {
          res[u[i]] = x[i];
          take[i] = x[i] > rmax;
          deg[i] = d;
        }
      }
    }
    block_tile_compact<kTargetItems>(take, deg, counter, [&](int i, uint32_t pos, unsigned long long eo) {
      F[pos] = u[i];
      eoff[pos] = (uint32_t)eo;
    });
  }
}

// value = p / S over the slot's live range, in place: a thread takes eight consecutive nodes (four 16-byte loads of
// each vector, four 16-byte stores), the last group of a range that is no multiple of eight node by node.  S >= alpha
// everywhere, and p = 0 stays 0.  Plain vector stores only.
__global__ __launch_bounds__(256) void k_target_finish(double* __restrict__ reserve, const double* __restrict__ surv,
                                                        uint32_t n) {
  const uint32_t tile = 256u * kTargetItems;
  const uint32_t n_tiles = (n + tile - 1) / tile;
  for (uint32_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const uint32_t v0 = tl * tile + threadIdx.x * kTargetItems;
    if (v0 + kTargetItems <= n) {
      double2* r2 = reinterpret_cast<double2*>(reserve + v0);
      const double2* s2 = reinterpret_cast<const double2*>(surv + v0);
      double2 p[kTargetItems / 2], s[kTargetItems / 2];
#pragma unroll
      for (int i = 0; i < kTargetItems / 2; ++i) {
        p[i] = r2[i];
        s[i] = s2[i];
      }
#pragma unroll
      for (int i = 0; i < kTargetItems / 2; ++i) {
        p[i].x = p[i].x / s[i].x;
        p[i].y = p[i].y / s[i].y;
        r2[i] = p[i];
      }
    } else {
      for (uint32_t v = v0; v < n; ++v) reserve[v] = reserve[v] / surv[v];
    }
  }
}

// a single target whose push ran no level (no in-edges, maybe isolated and beyond the live range): its own entry is
// the vector
__global__ void k_target_finish_one(double* __restrict__ reserve, const double* __restrict__ surv, uint32_t v) {
  reserve[v] = reserve[v] / surv[v];
}

int launch_target_init(pprhip_graph* g, const int32_t* d_id, const double* d_w, uint32_t count, int fbuf,
                       unsigned long long* d_counter, double alpha, double rmax) {
  if (!count) return PPRHIP_OK;
  const uint32_t tiles = (count + 256u * kTargetItems - 1) / (256u * kTargetItems);
  const uint32_t grid = std::min<uint32_t>(tiles, (uint32_t)g->gr->n_cus * 4u);
  hipLaunchKernelGGL(k_target_init, dim3(std::max(1u, grid)), dim3(256), 0, g->stream, d_id, d_w, count, g->gr->in_rp,
                     g->residue, g->reserve, g->F[fbuf], g->eoff[fbuf], d_counter, alpha, rmax);
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

// lone >= 0: only that entry (internal id); else the n first entries
int launch_target_finish(pprhip_graph* g, const double* d_survival, uint32_t n, int32_t lone) {
  if (lone >= 0) {
    hipLaunchKernelGGL(k_target_finish_one, dim3(1), dim3(1), 0, g->stream, g->reserve, d_survival, (uint32_t)lone);
  } else {
    if (!n) return PPRHIP_OK;
    const uint32_t tiles = (n + 256u * kTargetItems - 1) / (256u * kTargetItems);
    const uint32_t grid = std::min<uint32_t>(tiles, (uint32_t)g->gr->n_cus * 8u);
    hipLaunchKernelGGL(k_target_finish, dim3(std::max(1u, grid)), dim3(256), 0, g->stream, g->reserve, d_survival, n);
  }
  PPRHIP_CHECK_HIP(hipGetLastError());
  return PPRHIP_OK;
}

int init_kernels_target() {  // loads this file's code object on the current device (see init_kernels_push)
  hipFuncAttributes fa;
  PPRHIP_CHECK_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_target_finish)));
  return PPRHIP_OK;
}

}  // namespace pprhip
