// index.cpp — the inverted index of All-Pair-Backward-Search (pprhip_index): rows finished on the device and downloaded
// through a ring of pinned slots (index_from_device), or built from entries on the host (index_from_triples:
// finalize_rows), rows of several indexes put together (index_concat), and the pprhip_index_* ABI.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

struct pprhip_index {
  uint32_t n = 0;
  RawVec<uint64_t> offsets;
  RawVec<int32_t> targets;
  RawVec<double> values;
};

namespace {

// Host threads for the index finalisation: what the process may really use at once (lift.cpp: host_threads - CPU
// affinity and cgroup quota; the GPU boxes give a one-GPU job 16 of 256 hardware threads, and more threads than that
// are throttled, not added).
static unsigned finalise_threads() { return host_threads(); }

// Base_Whole_Graph.java:112-163: per source, k < 0 keeps insertion (target) order; k >= 0 keeps
// entries >= the k-th largest (all when fewer than k) sorted descending (stable: ties stay in
// target order).
void finalize_rows(uint32_t n, std::vector<Triple>& tr, int k, pprhip_index* ix) {
  ix->n = n;
  // bucket by source, then every bucket on its own: order by target, apply the k rule.  The bucketing is a two-level
  // counting sort so that it runs on all threads: entries go to 256 coarse ranges of sources first (per-thread
  // histograms, sequential writes), then every coarse range is sorted by source on its own (a working set of
  // n / 256 counters); one thread's scatter over all n sources was a third of the call at 32 M entries.
  const size_t N = tr.size();
  std::vector<uint64_t> start((size_t)n + 1, 0);
  std::vector<Triple> by_v(N);
  const unsigned hw = finalise_threads();
  const unsigned T = N < (1u << 16) ? 1u : hw;
  auto parallel = [&](unsigned parts, auto&& fn) {  // fn(part) for part in [0, parts), T threads
    std::atomic<unsigned> next{0};
    auto work = [&]() {
      for (unsigned p = next.fetch_add(1); p < parts; p = next.fetch_add(1)) fn(p);
    };
    std::vector<std::thread> th;
    for (unsigned w = 1; w < T; ++w) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
  };
  {
    constexpr unsigned kCoarse = 256;
    const uint32_t span = (uint32_t)(((uint64_t)n + kCoarse - 1) / kCoarse);  // sources per coarse range
    const unsigned chunks = T;
    std::vector<uint64_t> hist((size_t)chunks * kCoarse, 0);
    auto chunk_lo = [&](unsigned c) { return (size_t)((unsigned long long)N * c / chunks); };
    parallel(chunks, [&](unsigned c) {
      uint64_t* h = hist.data() + (size_t)c * kCoarse;
      for (size_t i = chunk_lo(c); i < chunk_lo(c + 1); ++i) h[(uint32_t)tr[i].v / span]++;
    });
    // coarse range b of chunk c starts at: all of ranges < b, then chunks < c of range b
    std::vector<uint64_t> base((size_t)chunks * kCoarse, 0), cstart(kCoarse + 1, 0);
    uint64_t run = 0;
    for (unsigned b = 0; b < kCoarse; ++b) {
      cstart[b] = run;
      for (unsigned c = 0; c < chunks; ++c) {
        base[(size_t)c * kCoarse + b] = run;
        run += hist[(size_t)c * kCoarse + b];
      }
    }
    cstart[kCoarse] = run;
    std::vector<Triple> coarse(N);
    parallel(chunks, [&](unsigned c) {
      uint64_t* at = base.data() + (size_t)c * kCoarse;
      for (size_t i = chunk_lo(c); i < chunk_lo(c + 1); ++i) coarse[at[(uint32_t)tr[i].v / span]++] = tr[i];
    });
    std::vector<Triple>().swap(tr);
    parallel(kCoarse, [&](unsigned b) {
      const uint32_t v_lo = std::min<uint64_t>((uint64_t)b * span, n), v_hi = std::min<uint64_t>((uint64_t)(b + 1) * span, n);
      if (v_lo >= v_hi) return;
      std::vector<uint64_t> cnt((size_t)(v_hi - v_lo) + 1, 0);
      for (uint64_t i = cstart[b]; i < cstart[b + 1]; ++i) cnt[(uint32_t)coarse[i].v - v_lo + 1]++;
      uint64_t acc = cstart[b];  // entries of sources below v_lo = entries of the coarse ranges below b
      for (uint32_t v = v_lo; v < v_hi; ++v) {
        start[v] = acc;
        acc += cnt[v - v_lo + 1];
        cnt[v - v_lo + 1] = start[v];  // becomes the write cursor of source v
      }
      for (uint64_t i = cstart[b]; i < cstart[b + 1]; ++i) by_v[cnt[(uint32_t)coarse[i].v - v_lo + 1]++] = coarse[i];
    });
    start[n] = N;
  }
  std::vector<uint64_t> kept((size_t)n + 1, 0);
  auto for_ranges = [&](auto&& fn) {
    std::vector<std::thread> th;
    for (unsigned w = 1; w < T; ++w) th.emplace_back(fn, (uint32_t)((uint64_t)n * w / T), (uint32_t)((uint64_t)n * (w + 1) / T));
    fn(0u, (uint32_t)((uint64_t)n / T));
    for (auto& x : th) x.join();
  };
  // pass 1: each bucket sorted by target; for k >= 0 the kept entries move to the bucket's front, by value
  for_ranges([&](uint32_t lo, uint32_t hi) {
    std::vector<double> tmp;
    for (uint32_t v = lo; v < hi; ++v) {
      Triple* b = by_v.data() + start[v];
      const size_t len = (size_t)(start[v + 1] - start[v]);
      if (len == 0) continue;
      std::sort(b, b + len, [](const Triple& x, const Triple& y) { return x.t < y.t; });
      if (k < 0) {
        kept[v + 1] = len;
        continue;
      }
      bool have = false;
      double kth = 0.0;
      if (k >= 1 && (size_t)k <= len) {
        tmp.resize(len);
        for (size_t j = 0; j < len; ++j) tmp[j] = b[j].p;
        std::nth_element(tmp.begin(), tmp.begin() + (k - 1), tmp.end(), std::greater<double>());
        kth = tmp[k - 1];
        have = true;
      }
      size_t w = 0;
      for (size_t j = 0; j < len; ++j)
        if (!have || b[j].p >= kth) b[w++] = b[j];
      std::stable_sort(b, b + w, [](const Triple& x, const Triple& y) { return x.p > y.p; });
      kept[v + 1] = w;
    }
  });
  for (uint32_t v = 0; v < n; ++v) kept[v + 1] += kept[v];
  ix->targets.resize(kept[n]);
  ix->values.resize(kept[n]);
  // pass 2: into the index arrays
  for_ranges([&](uint32_t lo, uint32_t hi) {
    for (uint32_t v = lo; v < hi; ++v) {
      const Triple* b = by_v.data() + start[v];
      const size_t len = (size_t)(kept[v + 1] - kept[v]);
      for (size_t j = 0; j < len; ++j) {
        ix->targets[kept[v] + j] = b[j].t;
        ix->values[kept[v] + j] = b[j].p;
      }
    }
  });
  ix->offsets.assign(kept.begin(), kept.end());
}

}  // namespace

namespace pprhip {
namespace detail {

// ---- device -> pageable host memory through a ring of pinned slots and copier threads
constexpr int kIxSlots = 8;
constexpr size_t kIxSlotBytes = 8u << 20;
constexpr int kIxCopiers = 4;

int ensure_ring(pprhip_graph* g) {  // the ring lives in g->ix_stage (kIxSlots * kIxSlotBytes of pinned memory)
  if (g->ix_stage && g->ix_stage_bytes >= kIxSlots * kIxSlotBytes) return PPRHIP_OK;
  if (g->ix_stage) (void)hipHostFree(g->ix_stage);
  g->ix_stage = nullptr;
  g->ix_stage_bytes = 0;
  if (hipHostMalloc(&g->ix_stage, kIxSlots * kIxSlotBytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    g->ix_stage = nullptr;
    return PPRHIP_ERR_OOM;  // (the caller falls back to a plain copy)
  }
  g->ix_stage_bytes = kIxSlots * kIxSlotBytes;
  return PPRHIP_OK;
}

int ring_download(pprhip_graph* g, const void* d_src, void* h_dst, size_t bytes) {
  if (!bytes) return PPRHIP_OK;
  if (bytes < 4 * kIxSlotBytes || ensure_ring(g) != PPRHIP_OK) {  // small, or no pinned memory to be had
    PPRHIP_CHECK_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, g->stream));
    PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    return PPRHIP_OK;
  }
  char* const ring = static_cast<char*>(g->ix_stage);
  hipEvent_t ev[kIxSlots] = {};
  for (int i = 0; i < kIxSlots; ++i)
    if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) {
      for (int j = 0; j < i; ++j) (void)hipEventDestroy(ev[j]);
      set_error("index download: no events");
      return PPRHIP_ERR_HIP;
    }
  const size_t n_chunks = (bytes + kIxSlotBytes - 1) / kIxSlotBytes;
  std::mutex mu;
  std::condition_variable cv;
  size_t issued = 0;                 // chunks whose copy into their slot has been queued
  size_t taken = 0;                  // next chunk a copier takes
  size_t freed[kIxSlots] = {};       // per slot: chunks of that slot moved on so far
  int err = PPRHIP_OK;
  const int device = g->gr->device;
  auto copier = [&] {
    (void)hipSetDevice(device);
    for (;;) {
      size_t c;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return taken < issued || taken >= n_chunks || err; });
        if (err || taken >= n_chunks) return;
        c = taken++;
      }
      const int slot = (int)(c % kIxSlots);
      const size_t off = c * kIxSlotBytes, len = std::min(kIxSlotBytes, bytes - off);
      const bool ok = hipEventSynchronize(ev[slot]) == hipSuccess;
      if (ok) std::memcpy(static_cast<char*>(h_dst) + off, ring + (size_t)slot * kIxSlotBytes, len);
      {
        std::lock_guard<std::mutex> lk(mu);
        if (!ok && !err) err = PPRHIP_ERR_HIP;
        freed[slot]++;
      }
      cv.notify_all();
    }
  };
  std::thread th[kIxCopiers];
  int n_th = 0;
  try {
    for (; n_th < kIxCopiers; ++n_th) th[n_th] = std::thread(copier);
  } catch (const std::system_error&) {  // (no exception leaves the C ABI; the copiers that did start go on)
  }
  if (n_th == 0) {  // no thread to be had: the plain copy
    for (int i = 0; i < kIxSlots; ++i) (void)hipEventDestroy(ev[i]);
    PPRHIP_CHECK_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, g->stream));
    PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    return PPRHIP_OK;
  }
  for (size_t c = 0; c < n_chunks; ++c) {
    const int slot = (int)(c % kIxSlots);
    {
      std::unique_lock<std::mutex> lk(mu);  // the slot's previous chunk has been moved on
      cv.wait(lk, [&] { return freed[slot] >= c / kIxSlots || err; });
      if (err) break;
    }
    const size_t off = c * kIxSlotBytes, len = std::min(kIxSlotBytes, bytes - off);
    const bool ok = hipMemcpyAsync(ring + (size_t)slot * kIxSlotBytes, static_cast<const char*>(d_src) + off, len,
                                   hipMemcpyDeviceToHost, g->stream) == hipSuccess &&
                    hipEventRecord(ev[slot], g->stream) == hipSuccess;
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!ok && !err) err = PPRHIP_ERR_HIP;
      if (ok) issued = c + 1;
    }
    cv.notify_all();
    if (!ok) break;
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    if (issued < n_chunks && !err) err = PPRHIP_ERR_HIP;
  }
  cv.notify_all();
  for (int i = 0; i < n_th; ++i) th[i].join();
  (void)hipStreamSynchronize(g->stream);
  for (int i = 0; i < kIxSlots; ++i) (void)hipEventDestroy(ev[i]);
  if (err) set_error("index: download of the sorted entries failed");
  return err;
}

// the entries in a device record store -> the index (rows of sources in [v_lo, v_hi)): row order and the k rule on the
// device (kernels_sort.hip: finalize_rows_device), then the three index arrays cross PCIe as they are - through the
// ring of pinned slots into the index's own (pageable, huge-page) arrays.  The host does no per-entry and no per-row
// work: round 3's k rule on the host's threads was 36 ms of R-MAT 22's 53 ms and 160 of R-MAT 24's 240, and its passes
// over all n rows cost a rank of a sharded job the same whatever its share of the entries.
int index_from_device(pprhip_graph* g, const TripleRec* rec, unsigned long long count, int k, uint32_t v_lo, uint32_t v_hi,
                      pprhip_index_t** out) {
  if (v_lo > v_hi || v_hi > g->gr->n) {
    set_error("index: source range [%u, %u) outside [0, %u)", v_lo, v_hi, g->gr->n);
    return PPRHIP_ERR_INVALID;
  }
  const bool dbg = hook_env("PPRHIP_APBS_DEBUG") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  std::unique_ptr<pprhip_index> ix(new (std::nothrow) pprhip_index());
  if (!ix) return PPRHIP_ERR_OOM;
  ix->n = g->gr->n;
  DeviceRows R;
  PPRHIP_TRY(finalize_rows_device(g, rec, count, k, v_lo, v_hi, &R));
  if (dbg) fprintf(stderr, "[index] rows finished on the device at %.1f ms (%llu of %llu entries kept)\n", ms(), R.entries, count);
  if (!R.offsets) {  // no entries: every row is empty
    ix->offsets.assign((size_t)g->gr->n + 1, 0);
    *out = ix.release();
    return PPRHIP_OK;
  }
  try {
    ix->offsets.resize((size_t)g->gr->n + 1);
    ix->targets.resize(R.entries);
    ix->values.resize(R.entries);
  } catch (const std::bad_alloc&) {  // (up to 12 bytes of HBM per entry must not stay behind)
    set_error("index: no host memory for %llu entries", R.entries);
    device_rows_free(&R);
    return PPRHIP_ERR_OOM;
  }
  int rc = ring_download(g, R.offsets, ix->offsets.data(), 8 * ((size_t)g->gr->n + 1));
  if (rc == PPRHIP_OK) rc = ring_download(g, R.values, ix->values.data(), 8 * (size_t)R.entries);
  if (rc == PPRHIP_OK) rc = ring_download(g, R.targets, ix->targets.data(), 4 * (size_t)R.entries);
  device_rows_free(&R);
  if (rc != PPRHIP_OK) return rc;
  if (dbg) fprintf(stderr, "[index] on the host at %.1f ms\n", ms());
  *out = ix.release();
  return PPRHIP_OK;
}

// index over all n sources from entries of any targets, rows outside [v_lo, v_hi) must not occur
int index_from_triples(uint32_t n, std::vector<Triple>& tr, int k, pprhip_index_t** out) {
  // entries may come from a device buffer, an exchange or a caller's arrays: a source or target outside [0, n) must
  // be an error here, not an out-of-range write in the bucketing below
  for (const Triple& x : tr)
    if (x.v < 0 || (uint32_t)x.v >= n || x.t < 0 || (uint32_t)x.t >= n) {
      set_error("index entry (source %d, target %d) outside [0, %u)", x.v, x.t, n);
      return PPRHIP_ERR_INVALID;
    }
  std::unique_ptr<pprhip_index> ix(new (std::nothrow) pprhip_index());
  if (!ix) return PPRHIP_ERR_OOM;
  finalize_rows(n, tr, k, ix.get());
  *out = ix.release();
  return PPRHIP_OK;
}

// rows of several indexes over disjoint source ranges, put together (no k rule to re-apply)
int index_concat(const std::vector<pprhip_index_t*>& parts, pprhip_index_t** out) {
  std::unique_ptr<pprhip_index> ix(new (std::nothrow) pprhip_index());
  if (!ix) return PPRHIP_ERR_OOM;
  const uint32_t n = parts[0]->n;
  ix->n = n;
  ix->offsets.assign((size_t)n + 1, 0);
  for (const pprhip_index_t* p : parts)
    for (uint32_t v = 0; v < n; ++v) ix->offsets[v + 1] += p->offsets[v + 1] - p->offsets[v];
  for (uint32_t v = 0; v < n; ++v) ix->offsets[v + 1] += ix->offsets[v];
  ix->targets.resize(ix->offsets[n]);
  ix->values.resize(ix->offsets[n]);
  std::vector<uint64_t> at(ix->offsets.begin(), ix->offsets.end() - 1);
  for (const pprhip_index_t* p : parts)
    for (uint32_t v = 0; v < n; ++v)
      for (uint64_t i = p->offsets[v]; i < p->offsets[v + 1]; ++i) {
        ix->targets[at[v]] = p->targets[i];
        ix->values[at[v]++] = p->values[i];
      }
  *out = ix.release();
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip


extern "C" {

int pprhip_index_merge(const pprhip_index_t* const* shards, int n_shards, int k, pprhip_index_t** merged_out) {
  if (!shards || n_shards < 1 || !merged_out) {
    set_error("pprhip_index_merge: bad arguments");
    return PPRHIP_ERR_INVALID;
  }
  if (!shards[0]) {
    set_error("pprhip_index_merge: shard 0 is null");
    return PPRHIP_ERR_INVALID;
  }
  const uint32_t n = shards[0]->n;
  std::vector<Triple> tr;
  for (int s = 0; s < n_shards; ++s) {
    if (!shards[s] || shards[s]->n != n) {
      set_error("pprhip_index_merge: shard %d does not match", s);
      return PPRHIP_ERR_INVALID;
    }
    for (uint32_t v = 0; v < n; ++v)
      for (uint64_t i = shards[s]->offsets[v]; i < shards[s]->offsets[v + 1]; ++i)
        tr.push_back({(int32_t)v, shards[s]->targets[i], shards[s]->values[i]});
  }
  try {
    return index_from_triples(n, tr, k, merged_out);
  } catch (const std::exception& e) {
    set_error("pprhip_index_merge: %s", e.what());
    return PPRHIP_ERR_OOM;
  }
}

int pprhip_index_from_arrays(uint32_t n, const uint64_t* offsets, const int32_t* targets, const double* values,
                             pprhip_index_t** index_out) {
  if (!offsets || !index_out || offsets[0] != 0 || (offsets[n] && (!targets || !values))) {
    set_error("pprhip_index_from_arrays: bad arguments");
    return PPRHIP_ERR_INVALID;
  }
  for (uint32_t v = 0; v < n; ++v)
    if (offsets[v + 1] < offsets[v]) {
      set_error("pprhip_index_from_arrays: offsets must be non-decreasing");
      return PPRHIP_ERR_INVALID;
    }
  for (uint64_t i = 0; i < offsets[n]; ++i)
    if (targets[i] < 0 || (uint32_t)targets[i] >= n) {
      set_error("pprhip_index_from_arrays: target %d at position %llu outside [0, %u)", targets[i],
                (unsigned long long)i, n);
      return PPRHIP_ERR_INVALID;
    }
  std::unique_ptr<pprhip_index> ix(new (std::nothrow) pprhip_index());
  if (!ix) return PPRHIP_ERR_OOM;
  ix->n = n;
  ix->offsets.assign(offsets, offsets + n + 1);
  ix->targets.assign(targets, targets + offsets[n]);
  ix->values.assign(values, values + offsets[n]);
  *index_out = ix.release();
  return PPRHIP_OK;
}

int pprhip_index_from_entries(uint32_t n, const int32_t* sources, const int32_t* targets, const double* values,
                              uint64_t count, int k, pprhip_index_t** index_out) {
  if (!index_out || (count && (!sources || !targets || !values))) {
    set_error("pprhip_index_from_entries: null argument");
    return PPRHIP_ERR_INVALID;
  }
  try {
    std::vector<Triple> tr(count);
    for (uint64_t i = 0; i < count; ++i) tr[i] = Triple{sources[i], targets[i], values[i]};
    return index_from_triples(n, tr, k, index_out);  // validates the ids, buckets by source, applies the k rule
  } catch (const std::exception& e) {
    set_error("pprhip_index_from_entries: %s", e.what());
    return PPRHIP_ERR_OOM;
  }
}

int pprhip_index_info(const pprhip_index_t* ix, uint32_t* n, uint64_t* entries) {
  if (!ix) {
    set_error("pprhip_index_info: null index");
    return PPRHIP_ERR_INVALID;
  }
  if (n) *n = ix->n;
  if (entries) *entries = ix->targets.size();
  return PPRHIP_OK;
}

int pprhip_index_arrays(const pprhip_index_t* ix, const uint64_t** offsets, const int32_t** targets,
                        const double** values) {
  if (!ix || !offsets || !targets || !values) {
    set_error("pprhip_index_arrays: null argument");
    return PPRHIP_ERR_INVALID;
  }
  *offsets = ix->offsets.data();
  *targets = ix->targets.data();
  *values = ix->values.data();
  return PPRHIP_OK;
}

void pprhip_index_destroy(pprhip_index_t* ix) { delete ix; }

}  // extern "C"
