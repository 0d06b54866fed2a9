// device_io.cpp — what talks to the handle's stream on the host's behalf: the kernel-timing switch and the calling
// thread's timer, the scopes that bracket setup kernels (SetupScope) and move a slot's kernels to the sweeps' stream
// (C8Scope), the mailbox read-backs (fetch_*), the query-end counters, the walk-phase launchers and the side-stream
// probe.  The level loop that reads back through these is levels.cpp, the workspaces they read graph.cpp, the
// entry points engine.cpp (shared declarations: engine_internal.hpp).
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace pprhip {

std::atomic<int> g_kernel_timing{-1};
bool kernel_timing_on() {
  int v = g_kernel_timing.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = hook_env("PPRHIP_KERNEL_TIMER");
    v = (e && e[0] == '1') ? 1 : 0;
    g_kernel_timing.store(v, std::memory_order_relaxed);
  }
  return v != 0;
}
int kernel_timing_level() {
  (void)kernel_timing_on();  // (decides on first use)
  return g_kernel_timing.load(std::memory_order_relaxed);
}

namespace detail {

thread_local KernelTimer g_timer_own;
thread_local KernelTimer* g_timer_cur = &g_timer_own;

SetupScope::SetupScope(pprhip_graph* g) : t(g_timer_cur->stream == g->stream ? g_timer_cur : nullptr) {
  if (t) t->begin(PPRHIP_KERNEL_QUERY_SETUP, 0);
}

C8Scope::C8Scope(pprhip_graph* g_, bool back_) : g(g_), back(back_) {
  if (!g->parent || !g->c8_via_parent || g->stream == g->parent->stream) return;
  for (auto& e : g->c8_ev)
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      e = nullptr;
      set_error("hipEventCreate failed (slot %d)", g->slot_index);
      rc = PPRHIP_ERR_HIP;
      return;
    }
  // (the slots share one stream: a wait for it is a wait for whatever another slot has just queued there, so a slot
  // that is known to have nothing pending - it comes out of a sweep, or stood waiting for its column - does not ask)
  if (!g->c8_settled && (hipEventRecord(g->c8_ev[0], g->stream) != hipSuccess ||
                         hipStreamWaitEvent(g->parent->stream, g->c8_ev[0], 0) != hipSuccess)) {
    set_error("slot %d: its stream could not be joined to the sweeps' stream", g->slot_index);
    rc = PPRHIP_ERR_HIP;
    return;
  }
  own = g->stream;
  g->stream = g->parent->stream;
  g->parent->batch->in_c8++;
  on = true;
}

int C8Scope::leave() {
  if (!on) return rc;
  on = false;
  g->stream = own;
  g->parent->batch->in_c8--;
  if (back && (hipEventRecord(g->c8_ev[1], g->parent->stream) != hipSuccess ||
               hipStreamWaitEvent(own, g->c8_ev[1], 0) != hipSuccess)) {
    set_error("slot %d: the sweeps' stream could not be joined to its stream", g->slot_index);
    rc = PPRHIP_ERR_HIP;
  }
  return rc;
}

// A few words the host needs before it can queue the next kernel: published by a kernel into mapped pinned memory and
// awaited by spinning on the sequence word (kernels_host.hip); after kSpinUs the thread stops spinning and blocks in
// hipStreamSynchronize, which is also where a faulted kernel is reported.  `bytes`: a multiple of 8.
int fetch_begin(pprhip_graph* g, const void* dev, size_t bytes, unsigned long long* seq_out) {
  if (!g->mail || bytes > sizeof(unsigned long long) * kMailWords || (bytes & 7)) {
    *seq_out = 0;  // fetch_end copies and synchronises
    return PPRHIP_OK;
  }
  *seq_out = ++g->mail_seq;
  return launch_publish(g, dev, (uint32_t)(bytes / 8), *seq_out);
}

int fetch_end(pprhip_graph* g, unsigned long long seq, const void* dev, void* host, size_t bytes) {
  if (seq == 0) {
    PPRHIP_CHECK_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, g->stream));
    PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    return PPRHIP_OK;
  }
  // A slot of the sequential batch driver waits here while a sweep runs on the compute stream: the driver's hook is
  // called between looks at the mailbox, so that the sweep's end is noticed - and the next sweep launched - at once
  // instead of after this slot's step (kernel trace: the compute stream waited 97 us per sweep for the host).
  pprhip_graph* const H = g->parent;
  const BatchState* bs = H ? H->batch : nullptr;
  const bool hooked = bs && bs->idle_hook;
  const double kSpinUs = hooked ? 2e6 : 60.0;
  const auto t0 = std::chrono::steady_clock::now();
  bool arrived = false;
  for (uint32_t spins = 0;; ++spins) {
    if (__atomic_load_n(&g->mail->seq, __ATOMIC_ACQUIRE) == seq) {
      arrived = true;
      break;
    }
    __builtin_ia32_pause();
    if (hooked && (spins & 7u) == 7u) bs->idle_hook(bs->idle_arg);
    if ((spins & 63u) == 63u &&
        std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > kSpinUs)
      break;
  }
  if (!arrived) {
    PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    if (H && H->stream != g->stream) PPRHIP_CHECK_HIP(hipStreamSynchronize(H->stream));  // (a C8Scope publication)
    if (__atomic_load_n(&g->mail->seq, __ATOMIC_ACQUIRE) != seq) {
      set_error("fetch_small: the stream drained without the published words (sequence %llu, expected %llu)",
                (unsigned long long)g->mail->seq, seq);
      return PPRHIP_ERR_STATE;
    }
  }
  std::memcpy(host, g->mail->words, bytes);
  return PPRHIP_OK;
}

int fetch_small(pprhip_graph* g, const void* dev, void* host, size_t bytes) {
  unsigned long long seq = 0;
  PPRHIP_TRY(fetch_begin(g, dev, bytes, &seq));
  return fetch_end(g, seq, dev, host, bytes);
}

int device_sum(pprhip_graph* g, const double* x, double* out, uint32_t count) {
  poll_idle(g);
  {
    SetupScope setup(g);
    PPRHIP_TRY(launch_sum(g, x, count ? count : act_n(g)));
  }
  PPRHIP_TRY(fetch_small(g, &g->ctr->sum_out, &g->h_ctr->sum_out, sizeof(double)));
  *out = g->h_ctr->sum_out;
  return PPRHIP_OK;
}

// The counters a query only needs once, at its end, in one copy: dead-end pops of the push, and what the walk phases
// run since the workspace was reset counted on the device (steps, walks, sources: adjacent in DevCounters).
int read_dead_pops(pprhip_graph* g, pprhip_stats_t& st) {
  poll_idle(g);
  static_assert(offsetof(DevCounters, share_stored) == offsetof(DevCounters, dead_pops) + 64, "one copy for the nine");
  PPRHIP_TRY(fetch_small(g, &g->ctr->dead_pops, &g->h_ctr->dead_pops, 9 * sizeof(unsigned long long)));
  st.walk_loads = g->h_ctr->walk_loads;
  st.walk_load_lanes = g->h_ctr->walk_lanes;
  st.push_bytes += 16ull * (g->h_ctr->dead_pops - st.dead_end_pops);
  st.dead_end_pops = g->h_ctr->dead_pops;
  // cumulative over the query's walk phases: what is new since the last read goes into the statistics
  const uint64_t steps = g->h_ctr->walk_steps, walks = g->h_ctr->walks_total, srcs = g->h_ctr->sources_total;
  if (steps >= st.walk_steps && walks >= st.walks && srcs >= st.mc_sources) {
    // a walk served from the walk index (whole-graph queries: one walk phase, so the counter is the phase's) moves its
    // 4-byte terminal and its 8-byte deposit instead of a live walk's 16 bytes, and the plan is streamed a second time
    // (DESIGN.md §2 "Walk index")
    const uint64_t served = std::min<uint64_t>(g->h_ctr->walks_served, walks - st.walks);
    // the call's terminal cache (WalkShare): a walk it answered moves its 4-byte cell and its 8-byte deposit, a walk
    // that filled a cell the probe and the store on top of a live walk's 16 bytes
    const uint64_t shared = std::min<uint64_t>(g->h_ctr->share_served, walks - st.walks - served);
    const uint64_t more = 12ull * (steps - st.walk_steps) + 16ull * (walks - st.walks - served - shared) +
                          12ull * (served + shared) + 8ull * g->h_ctr->share_stored +
                          (served ? 24ull : 12ull) * (srcs - st.mc_sources);
    // a walk that left a deposit record (WalkDeposit) writes 12 bytes in place of its 8-byte add; the records are read
    // by the count (4), read and written by the scatter (12 + 12) and read by the sum (12): 44 bytes more per such walk
    uint64_t recorded = 0;
    if (g->walk_dep_cap && walks - st.walks >= g->walk_dep_min) recorded = std::min<uint64_t>(walks - st.walks, g->walk_dep_cap);
    g->walk_dep_cap = g->walk_dep_min = 0;
#ifdef PPRHIP_TEST_HOOKS
    if (hook_env("PPRHIP_WALK_SHARE_LOG"))  // measurement switch: a line per finished query, in completion order
      fprintf(stderr, "[walk-share] walks %llu served %llu stored %llu steps %llu\n", (unsigned long long)(walks - st.walks),
              (unsigned long long)g->h_ctr->share_served, (unsigned long long)g->h_ctr->share_stored,
              (unsigned long long)(steps - st.walk_steps));
#endif
    st.mc_bytes += more + 44ull * recorded;
    ktimer().add_bytes(PPRHIP_KERNEL_WALK, more + 44ull * recorded);
    st.walk_steps = steps;
    st.walks = walks;
    st.mc_sources = srcs;
  }
  return PPRHIP_OK;
}

// Walk phase shared by FORA whole-graph (variant 0) and top-k (variant 1): plan and walks are launched back to back,
// the walk kernel reads the plan's counts on the device (no host round trip inside the phase; the counts reach the
// statistics through read_dead_pops at the end of the query).  omega_dev > 0: the plan also derives rsum and the walk
// budget on the device from the residue sum a device_sum / launch_sum has just left (rsum, nrw are ignored; nrw_bound is
// the largest budget possible, for the range check).
// The walk phase in two halves (a caller may queue other work between them, or run the plan on another stream):
// the plan of the residue entries, and the walk kernel that runs the latest plan.
int launch_walk_plan(pprhip_graph* g, int variant, double alpha, double rsum, long long nrw, double* target, double omega_dev,
                     const double* copy_src, double* copy_dst) {
  poll_idle(g);
  // what the host knows about the walk count sizes the grid: the budget itself (every residue entry adds at most one
  // walk to it), or - with the budget derived on the device - nothing
  g->walk_hint = omega_dev > 0.0 ? 0ull : (unsigned long long)nrw + act_n(g);
  const double bound = omega_dev > 0.0 ? omega_dev : (double)nrw;
  if (bound + (double)g->gr->n >= (double)(1ull << kPackShift)) {
    set_error("walk budget %.0f exceeds the engine's 2^36 walk limit", bound);
    return PPRHIP_ERR_INVALID;
  }
  SetupScope setup(g);
  return launch_mc_plan(g, variant, alpha, rsum, (double)nrw, omega_dev, target, copy_src, copy_dst);
}

int launch_walk_run(pprhip_graph* g, int variant, double alpha, uint64_t seed, uint32_t stream, double* target) {
  poll_idle(g);
  ktimer().begin(PPRHIP_KERNEL_WALK, 0);  // (its bytes are added when the counters are read)
  // Whole-graph FORA walks (variant 0: stream 0, forced first hop, walk indices 0 .. omega_i - 1 per residue node) are
  // read from the handle's walk index when it was built at this alpha and seed, bit for bit; everything else walks.
  const WalkIndex* ix = g->gr->widx;
  // ... and a slot of a batched call reads and fills the call's terminal cache when the call keeps one for this seed
  // (walk_share_begin; a handle with a walk index has none)
  const WalkShare* ws = g->parent && g->parent->batch ? g->parent->batch->share : nullptr;
  if (variant == 0 && stream == 0 && ix && std::memcmp(&ix->alpha, &alpha, sizeof alpha) == 0 && ix->seed == seed) {
    PPRHIP_TRY(launch_mc_walk_indexed(g, ix, alpha, seed, target));
  } else if (variant == 0 && stream == 0 && ws && ws->on && ws->seed == seed &&
             std::memcmp(&ws->alpha, &alpha, sizeof alpha) == 0) {
    PPRHIP_CHECK_HIP(hipStreamWaitEvent(g->stream, ws->cleared, 0));  // (the call's clear ran on the handle's stream)
    // ... and leaves its deposits as records when it runs on the call's one walk stream (one set of buffers per handle)
    const hipStream_t walk_stream = g->parent->batch->walk_stream;
    const WalkDeposit* dep = walk_stream && g->stream == walk_stream && ws->dep.on ? &ws->dep : nullptr;
    g->walk_dep_cap = dep ? dep->a.cap : 0ull;
    g->walk_dep_min = dep ? dep->a.min_walks : 0ull;
    PPRHIP_TRY(launch_mc_walk_shared(g, ws, alpha, seed, target, dep));
  } else
    PPRHIP_TRY(launch_mc_walk(g, alpha, seed, stream, variant == 0 ? 1 : 0, target));
  ktimer().end();
  return PPRHIP_OK;
}

int run_walk_phase(pprhip_graph* g, int variant, double alpha, double rsum, long long nrw, uint64_t seed, uint32_t stream,
                   double* target, pprhip_stats_t& st, double omega_dev) {
  (void)st;
  PPRHIP_TRY(launch_walk_plan(g, variant, alpha, rsum, nrw, target, omega_dev));
  return launch_walk_run(g, variant, alpha, seed, stream, target);
}

// A stream that really runs beside the handle's compute stream.  The runtime spreads streams over a few in-order
// hardware queues, and which streams share one depends on what else the process has created: a stream that lands on
// the compute stream's queue never overlaps it (fetch_pipe.cpp: FetchPipe, tools/exp/copy_overlap.py: kernels ran during
// 0.0 % of the copies' time).  So candidates are created - plain ones first, then of the other priorities - and each
// is tried: a kernel holds the compute stream for a moment, a one-word k_publish goes to the candidate, and the
// candidate is taken if the word arrives while the hold kernel still runs.  Rejected candidates stay alive until the
// search ends, so that the next one lands elsewhere.  *out stays null when none ran beside.
int make_side_stream(pprhip_graph* g, hipStream_t* out, hipStream_t also) {
  *out = nullptr;
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  HostMail* probe = nullptr;
  HostMail* probe_dev = nullptr;
  if (alloc_pinned((void**)&probe, sizeof(HostMail), hipHostMallocMapped) != PPRHIP_OK ||
      hipHostGetDevicePointer((void**)&probe_dev, probe, 0) != hipSuccess) {
    (void)hipGetLastError();
    if (probe) (void)hipHostFree(probe);
    return PPRHIP_ERR_OOM;
  }
  hipEvent_t held = nullptr, held2 = nullptr;
  if (hipEventCreateWithFlags(&held, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&held2, hipEventDisableTiming) != hipSuccess) {
    if (held) (void)hipEventDestroy(held);
    (void)hipHostFree(probe);
    return PPRHIP_ERR_HIP;
  }
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  if (also) PPRHIP_CHECK_HIP(hipStreamSynchronize(also));
  const int prios[] = {0, 0, 0, 0, prio_lo, prio_hi, prio_lo, prio_hi};
  std::vector<hipStream_t> rejected;
  unsigned long long seq = 0;
  for (int p : prios) {
    hipStream_t cand = nullptr;
    const hipError_t ce = p == 0 ? hipStreamCreateWithFlags(&cand, hipStreamNonBlocking)
                                 : hipStreamCreateWithPriority(&cand, hipStreamNonBlocking, p);
    if (ce != hipSuccess) break;
    bool beside = false;
    ++seq;
    hipStream_t own = g->stream;
    HostMail *m = g->mail, *md = g->mail_dev;
    const bool also_held = !also || (launch_hold(also, 30000ull) == PPRHIP_OK && hipEventRecord(held2, also) == hipSuccess);
    if (also_held && launch_hold(own, 30000ull) == PPRHIP_OK && hipEventRecord(held, own) == hipSuccess) {  // ~0.3 ms at 100 MHz
      g->stream = cand;
      g->mail = probe;
      g->mail_dev = probe_dev;
      const int rc = launch_publish(g, &g->ctr->sum_out, 1, seq);
      g->stream = own;
      g->mail = m;
      g->mail_dev = md;
      if (rc == PPRHIP_OK) {
        const auto t0 = std::chrono::steady_clock::now();
        while (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() < 150.0) {
          if (__atomic_load_n(&probe->seq, __ATOMIC_ACQUIRE) == seq) {
            // arrived while the hold kernel(s) still run
            beside = hipEventQuery(held) == hipErrorNotReady && (!also || hipEventQuery(held2) == hipErrorNotReady);
            break;
          }
          __builtin_ia32_pause();
        }
      }
    }
    (void)hipStreamSynchronize(own);
    if (also) (void)hipStreamSynchronize(also);
    (void)hipStreamSynchronize(cand);
    if (beside) {
      *out = cand;
      break;
    }
    rejected.push_back(cand);
  }
  for (hipStream_t r : rejected) (void)hipStreamDestroy(r);
  (void)hipEventDestroy(held);
  (void)hipEventDestroy(held2);
  (void)hipHostFree(probe);
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip
