// stream.cpp — the query stream: the one-thread batch driver (batch_driver.hpp: SlotDriver) behind a submit / wait pair.
// A synchronous call of q queries ends with a drain: its last queries finish at different times, the slots they leave
// stay empty, and a sweep costs the same for 2 busy columns as for 16 (config #4's 50-query call, PPR.java:179: 0.90
// of the 128-query rate).  A stream keeps one driver thread on the handle; the slots a submission's last queries leave
// take the next submission's first ones, so queries that arrive continuously - a harness that calls Gen_Util's loop
// again and again, a server - always find sixteen columns busy.  Every query runs exactly as
// pprhip_fora_batch_single_source would run it (same seed, same tuning, same result).
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include "batch_driver.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace {

struct StreamJob : BatchJob {
  std::vector<int32_t> own_srcs;  // (the caller's array need not outlive the submit call)
  uint64_t ticket = 0;
  int finished = 0;
  bool done = false;
  std::chrono::steady_clock::time_point t0;
};

}  // namespace

struct pprhip_stream {
  pprhip_graph* g = nullptr;
  double eps = 0.0;
  pprhip_fora_conf_t conf;
  int k = 0;
  std::mutex mu;
  std::condition_variable cv_work, cv_done;
  std::deque<std::shared_ptr<StreamJob>> pending;           // submissions with queries still to start
  std::map<uint64_t, std::shared_ptr<StreamJob>> open;      // ticket -> submission, until it has been waited for
  uint64_t next_ticket = 1;
  bool closing = false;
  int err = PPRHIP_OK;
  std::string errmsg;
  std::thread driver;
};

namespace {

void stream_fail(pprhip_stream* s, int rc) {
  std::lock_guard<std::mutex> lk(s->mu);
  if (s->err == PPRHIP_OK) {
    s->err = rc;
    s->errmsg = get_error();
  }
  s->pending.clear();
  for (auto& kv : s->open) kv.second->done = true;
  s->cv_done.notify_all();
}

void stream_driver(pprhip_stream* s) {
  pprhip_graph* P = s->g;
  if (hipSetDevice(P->gr->device) != hipSuccess) {
    set_error("hipSetDevice(%d) failed in the stream driver", P->gr->device);
    stream_fail(s, PPRHIP_ERR_HIP);
    return;
  }
  KernelTimer quiet;  // nobody reads kernel-class times of a stream: record no events at all
  quiet.off = true;
  KernelTimer* const saved = g_timer_cur;
  g_timer_cur = &quiet;
  std::unique_ptr<SlotDriver> Dp(new (std::nothrow) SlotDriver());
  if (!Dp) {
    set_error("query stream: no memory for the driver's state");
    stream_fail(s, PPRHIP_ERR_OOM);
    g_timer_cur = saved;
    return;
  }
  SlotDriver& D = *Dp;
  (void)D.open(P, true, true);
  hipStream_t side = D.side;
  // test switch: PPRHIP_STREAM_FAULT_AT=<n> makes the driver fail when it is about to start the stream's n-th query
  // (0-based), as a failing kernel launch would: every open and later submission ends with the driver's error
  long fault_at = -1, started = 0;
  if (const char* fe = hook_env("PPRHIP_STREAM_FAULT_AT")) fault_at = atol(fe);
  bool injected = false;
  D.next = [&](BatchJob** job, int* i) {
    if (fault_at >= 0 && started == fault_at) {
      injected = true;
      return false;
    }
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->pending.empty()) return false;
    StreamJob* J = s->pending.front().get();
    *job = J;
    *i = J->next_query.fetch_add(1);
    if (*i + 1 >= J->q) s->pending.pop_front();  // (the open map keeps the submission alive)
    ++started;
    if (*i == 0) {
      // A submission's first query: with no other query in flight its queries get the terminal cache for their seed.
      // One that starts while an earlier one is still running shares that one's cache when the seeds agree and walks
      // on its own otherwise (launch_walk_run compares seeds): the cache is never cleared under a running walk kernel.
      bool idle = true;
      for (int w = 0; w < D.n_ws && idle; ++w) idle = D.runs[w].query < 0;
      if (idle) share_walks_of(*J);
    }
    return true;
  };
  D.done = [&](BatchJob* job) {
    StreamJob* J = static_cast<StreamJob*>(job);
    std::lock_guard<std::mutex> lk(s->mu);
    if (++J->finished == J->q) {
      J->sum.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - J->t0).count();
#ifdef PPRHIP_TEST_HOOKS
      (void)take_apply_counts(P, J->sum);  // (test switch: what the sweeps up to here counted on dead-end tiles)
#endif
      J->done = true;
      s->cv_done.notify_all();
    }
  };
  const int rc = D.run("query stream", " in the driver thread", [&](int busy) -> int {
    if (injected) {
      set_error("query stream: injected failure before query %ld (PPRHIP_STREAM_FAULT_AT)", fault_at);
      return PPRHIP_ERR_STATE;
    }
    if (busy == 0) {
      std::unique_lock<std::mutex> lk(s->mu);
      s->cv_work.wait(lk, [&] { return s->closing || !s->pending.empty(); });
      if (s->pending.empty()) return SlotDriver::kStop;  // closing, and nothing left to start or in flight
    }
    return SlotDriver::kGoOn;
  });
  // Drain before anybody is woken: a waiter that returns the error may free its result store or its output block at
  // once, and copies or selections of other slots' queries can still be queued against those buffers.
  (void)hipStreamSynchronize(P->stream);
  D.teardown();
  if (P->batch->share) P->batch->share->on = false;
  if (P->batch->walk_stream) (void)hipStreamSynchronize(P->batch->walk_stream);
  if (side && side != P->stream && side != P->batch->walk_stream) (void)hipStreamSynchronize(side);
  if (rc != PPRHIP_OK) stream_fail(s, rc);
  g_timer_cur = saved;
}

int stream_error(pprhip_stream* s, const char* fn) {  // (s->mu held)
  set_error("%s: the stream has failed: %s", fn, s->errmsg.c_str());
  return s->err;
}

}  // namespace

int pprhip_fora_stream_open(pprhip_graph_t* g, double eps, const pprhip_fora_conf_t* conf, int k,
                            pprhip_stream_t** stream_out) {
  PPRHIP_TRY(check_positive(eps, "pprhip_fora_stream_open", "eps"));
  PPRHIP_TRY(check_conf(conf, "pprhip_fora_stream_open", false));
  PPRHIP_TRY(check_graph(g, "pprhip_fora_stream_open"));
  if (!stream_out || !conf || !(eps > 0.0) || k < 0) {
    set_error("pprhip_fora_stream_open: bad arguments (eps=%g k=%d)", eps, k);
    return PPRHIP_ERR_INVALID;
  }
  PPRHIP_TRY(ensure_batch(g));
  std::unique_ptr<pprhip_stream> s(new (std::nothrow) pprhip_stream());
  if (!s) return PPRHIP_ERR_OOM;
  s->g = g;
  s->eps = eps;
  s->conf = *conf;
  s->k = k;
  PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
  g->stream_open = true;
  g->stream_obj = s.get();
  try {
    s->driver = std::thread(stream_driver, s.get());
  } catch (...) {
    g->stream_open = false;
    g->stream_obj = nullptr;
    set_error("pprhip_fora_stream_open: no thread for the driver");
    return PPRHIP_ERR_OOM;
  }
  *stream_out = s.release();
  return PPRHIP_OK;
}

int pprhip_fora_stream_submit(pprhip_stream_t* s, const int32_t* srcs, int q, uint64_t seed, pprhip_results_t* keep,
                              int keep_first, int32_t* ids_out, double* vals_out, int* n_out, uint64_t* ticket_out) {
  if (!s || !ticket_out || q < 1 || !srcs || (s->k > 0 && (!ids_out || !vals_out)) || keep_first < 0) {
    set_error("pprhip_fora_stream_submit: bad arguments (q=%d)", q);
    return PPRHIP_ERR_INVALID;
  }
  if (keep && (keep->g != s->g || (long long)keep_first + q > keep->capacity)) {
    set_error("pprhip_fora_stream_submit: the result store belongs to another graph or holds %d < %d + %d queries",
              keep->capacity, keep_first, q);
    return PPRHIP_ERR_INVALID;
  }
  if (!s->g) {
    set_error("pprhip_fora_stream_submit: the stream's graph has been destroyed");
    return PPRHIP_ERR_STATE;
  }
  for (int i = 0; i < q; ++i) PPRHIP_TRY(check_node(s->g, srcs[i], "pprhip_fora_stream_submit"));
  std::shared_ptr<StreamJob> J;
  try {
    J = std::make_shared<StreamJob>();
    J->own_srcs.assign(srcs, srcs + q);
  } catch (const std::bad_alloc&) {
    return PPRHIP_ERR_OOM;
  }
  J->P = s->g;
  J->srcs = J->own_srcs.data();
  J->q = q;
  J->eps = s->eps;
  J->conf = &s->conf;
  J->seed = seed;
  J->k = s->k;
  J->ids_out = ids_out;
  J->vals_out = vals_out;
  J->n_out = n_out;
  J->keep = keep;
  J->keep_first = keep_first;
  J->t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> lk(s->mu);
  if (s->err != PPRHIP_OK) return stream_error(s, "pprhip_fora_stream_submit");
  if (s->closing) {
    set_error("pprhip_fora_stream_submit: the stream is closing");
    return PPRHIP_ERR_STATE;
  }
  J->ticket = s->next_ticket;
  try {  // (no exception leaves the C ABI)
    s->open[J->ticket] = J;
    s->pending.push_back(J);
  } catch (const std::bad_alloc&) {
    s->open.erase(J->ticket);
    set_error("pprhip_fora_stream_submit: out of host memory");
    return PPRHIP_ERR_OOM;
  }
  s->next_ticket++;
  if (keep && keep->count < keep_first + q) keep->count = keep_first + q;
  *ticket_out = J->ticket;
  s->cv_work.notify_one();
  return PPRHIP_OK;
}

int pprhip_fora_stream_wait(pprhip_stream_t* s, uint64_t ticket, pprhip_stats_t* stats_sum) {
  if (!s) {
    set_error("pprhip_fora_stream_wait: null stream");
    return PPRHIP_ERR_INVALID;
  }
  std::unique_lock<std::mutex> lk(s->mu);
  auto it = s->open.find(ticket);
  if (it == s->open.end()) {
    set_error("pprhip_fora_stream_wait: no open submission with ticket %llu", (unsigned long long)ticket);
    return PPRHIP_ERR_INVALID;
  }
  std::shared_ptr<StreamJob> J = it->second;
  s->cv_done.wait(lk, [&] { return J->done; });
  s->open.erase(ticket);
  if (s->err != PPRHIP_OK) return stream_error(s, "pprhip_fora_stream_wait");
  if (stats_sum) *stats_sum = J->sum;
  return PPRHIP_OK;
}

// Ends the driver thread and takes the stream off its graph; the stream object stays (a later close frees it).
static int stream_shutdown(pprhip_stream* s) {
  pprhip_graph* g = s->g;
  if (!g) return s->err;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    s->closing = true;
    s->cv_work.notify_all();
  }
  if (s->driver.joinable()) s->driver.join();  // every submitted query has finished (or the stream has failed)
  g->stream_open = false;
  g->stream_obj = nullptr;
  s->g = nullptr;
  if (s->err != PPRHIP_OK) {
    (void)hipSetDevice(g->gr->device);
    free_batch(g);  // slots may hold half-pushed levels: the next batched call builds clean ones
  }
  return s->err;
}

namespace pprhip {
namespace detail {
// pprhip_graph_destroy on a handle whose stream is still open: the driver thread uses the handle, so it ends first.  The
// stream object is not freed here - its owner may still call pprhip_fora_stream_close on it (which then only frees it).
void stream_detach(void* stream_obj) {
  pprhip_stream* s = static_cast<pprhip_stream*>(stream_obj);
  (void)stream_shutdown(s);
  std::lock_guard<std::mutex> lk(s->mu);
  if (s->err == PPRHIP_OK) {
    s->err = PPRHIP_ERR_STATE;
    s->errmsg = "the stream's graph has been destroyed";
  }
  for (auto& kv : s->open) kv.second->done = true;
  s->cv_done.notify_all();
}
}  // namespace detail
}  // namespace pprhip

int pprhip_fora_stream_close(pprhip_stream_t* s) {
  if (!s) return PPRHIP_OK;
  const bool attached = s->g != nullptr;
  const int rc = stream_shutdown(s);
  int out = PPRHIP_OK;
  if (attached && rc != PPRHIP_OK) {
    set_error("pprhip_fora_stream_close: the stream had failed: %s", s->errmsg.c_str());
    out = rc;
  }
  delete s;
  return out;
}
