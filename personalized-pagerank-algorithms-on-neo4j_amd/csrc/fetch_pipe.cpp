// fetch_pipe.cpp — FetchPipe (engine_internal.hpp): delivery of a batched call's result vectors to the caller's host
// memory while the batch keeps running.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

int pprhip::detail::FetchPipe::ensure(pprhip_graph* parent) {
  if (cs) return PPRHIP_OK;
  P = parent;
  n = parent->gr->n;
  for (int e = 0; e < kRing; ++e) {
    PPRHIP_TRY(alloc_dev((void**)&dev[e], sizeof(double) * n));
    PPRHIP_CHECK_HIP(hipHostMalloc((void**)&pin[e], sizeof(double) * std::max<size_t>(n, 1), hipHostMallocDefault));
    PPRHIP_CHECK_HIP(hipEventCreateWithFlags(&ready[e], hipEventDisableTiming));
    PPRHIP_CHECK_HIP(hipEventCreateWithFlags(&done[e], hipEventDisableTiming));
  }
  // The copy stream has to sit on another hardware queue than the compute stream: on a shared queue no copy ever
  // overlapped a kernel (tools/exp/copy_overlap.py: kernels ran during 0.0 % of the copies' time).  make_side_stream
  // tries candidates until one runs beside the compute stream; without one, a plain stream (copies then run between
  // kernels, as before round 3).
  PPRHIP_TRY(make_side_stream(parent, &cs));
  if (!cs) PPRHIP_CHECK_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));  // last: marks the pipe complete
  return PPRHIP_OK;
}

void pprhip::detail::FetchPipe::start() {
  closing = false;
  err = 0;
  pending = 0;
  work.clear();
  free_q.clear();
  for (int e = 0; e < kRing; ++e) free_q.push_back(e);
  for (int t = 0; t < kCopiers; ++t) copiers[t] = std::thread(&FetchPipe::copier, this);
}

void pprhip::detail::FetchPipe::copier() {
  (void)hipSetDevice(P->gr->device);
  for (;;) {
    Item it;
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return !work.empty() || (closing && pending == 0); });
      if (work.empty()) return;  // closing and drained
      it = work.front();
      work.pop_front();
    }
    // (the item was queued by the copy stream's host callback: the vector is in pin[it.e]; copiers make no HIP call)
    std::memcpy(it.dst, pin[it.e], sizeof(double) * n);
    std::lock_guard<std::mutex> lk(mu);
    free_q.push_back(it.e);
    cv.notify_all();
  }
}

// host callback of the copy stream: the vector of ring entry e has reached its pinned buffer
void pprhip::detail::FetchPipe::on_copied(void* p) {
  Arrival* a = static_cast<Arrival*>(p);
  {
    std::lock_guard<std::mutex> lk(a->pipe->mu);
    a->pipe->work.push_back(a->item);
    a->pipe->pending--;
  }
  a->pipe->cv.notify_all();
  delete a;
}

int pprhip::detail::FetchPipe::submit(pprhip_graph* S, const double* dev_vec, double* dst) {
  int e;
  {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !free_q.empty() || err; });
    if (err) {
      set_error("delivery of a result vector failed (copy stream)");
      return err;
    }
    e = free_q.front();
    free_q.pop_front();
  }
  // A failure from here on hands the ring entry back and marks the pipe failed (finish() then stops waiting for
  // callbacks that may never run).  No HIP call is made with `mu` held: the copy stream's callback takes `mu` on a
  // thread of the runtime, and a HIP call that waited for work queued behind a pending callback would never return.
  auto fail = [&](int rc) {
    {
      std::lock_guard<std::mutex> lk(mu);
      free_q.push_back(e);
      if (!err) err = rc;
    }
    cv.notify_all();
    return rc;
  };
  int rc = PPRHIP_OK;
  if (S->gr->relabeled) {  // back to the caller's ids: out[old] = x[old2new[old]]
    rc = launch_permute_out(S, dev_vec, dev[e]);
  } else if (hipMemcpyAsync(dev[e], dev_vec, sizeof(double) * n, hipMemcpyDeviceToDevice, S->stream) != hipSuccess) {
    set_error("delivery of a result vector failed (staging copy)");
    rc = PPRHIP_ERR_HIP;
  }
  if (rc == PPRHIP_OK && hipEventRecord(ready[e], S->stream) != hipSuccess) {
    set_error("delivery of a result vector failed (event)");
    rc = PPRHIP_ERR_HIP;
  }
  if (rc != PPRHIP_OK) return fail(rc);
  Arrival* a = new (std::nothrow) Arrival{this, Item{e, dst}};
  if (!a) return fail(PPRHIP_ERR_OOM);
  {
    // the copy stream is shared by the slots' threads: its three calls stay together
    std::lock_guard<std::mutex> order(cs_mu);
    if (hipStreamWaitEvent(cs, ready[e], 0) != hipSuccess ||
        hipMemcpyAsync(pin[e], dev[e], sizeof(double) * n, hipMemcpyDeviceToHost, cs) != hipSuccess) {
      set_error("delivery of a result vector failed (copy stream)");
      delete a;
      return fail(PPRHIP_ERR_HIP);
    }
    {
      std::lock_guard<std::mutex> lk(mu);
      pending++;
    }
    if (hipLaunchHostFunc(cs, &FetchPipe::on_copied, a) != hipSuccess) {  // no callback will run for this entry
      set_error("delivery of a result vector failed (host callback)");
      {
        std::lock_guard<std::mutex> lk(mu);
        pending--;
      }
      delete a;
      return fail(PPRHIP_ERR_HIP);
    }
  }
  return PPRHIP_OK;
}

int pprhip::detail::FetchPipe::finish() {
  // the copy stream drains first (its callbacks queue the last vectors), then the copiers
  const bool drained = !cs || hipStreamSynchronize(cs) == hipSuccess;
  {
    std::lock_guard<std::mutex> lk(mu);
    if (!drained && !err) err = PPRHIP_ERR_HIP;
    closing = true;
    if (err) pending = 0;  // a failed copy stream may never run its callbacks: the copiers must not wait for them
  }
  cv.notify_all();
  for (int t = 0; t < kCopiers; ++t)
    if (copiers[t].joinable()) copiers[t].join();
  if (err) set_error("delivery of a result vector failed (copy stream)");
  return err;
}

void pprhip::detail::FetchPipe::destroy() {
  for (int e = 0; e < kRing; ++e) {
    if (dev[e]) (void)hipFree(dev[e]);
    if (pin[e]) (void)hipHostFree(pin[e]);
    if (ready[e]) (void)hipEventDestroy(ready[e]);
    if (done[e]) (void)hipEventDestroy(done[e]);
    dev[e] = pin[e] = nullptr;
    ready[e] = done[e] = nullptr;
  }
  if (cs) (void)hipStreamDestroy(cs);
  cs = nullptr;
}
