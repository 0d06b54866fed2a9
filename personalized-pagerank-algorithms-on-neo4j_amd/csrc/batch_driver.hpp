// batch_driver.hpp — what the batched call (batch.cpp) and the query stream (stream.cpp) share: the batched sweep's
// launch / collect, a query's begin / finish on a workspace, and the one-thread driver (SlotDriver).
#pragma once

#include <chrono>
#include <cstdio>
#include <functional>
#include <string>

#include "run.hpp"

namespace pprhip {
namespace detail {

// One batched dense level for the slots flagged in `active`.  The caller holds the sweep exclusively (sequential
// driver, or BatchSync::sweeping).
// launch: stages the slots' arguments, orders the parent stream behind the slots' prepare work, queues one batched sweep
// and the read-back of its counters; P->c8cur names the array the NEXT sweep reads from here on, so that whatever is
// queued on the parent's stream after this point - another slot's prepared level (C8Scope) - lands where that sweep
// will look.  collect: waits for the counters and does the slots' bookkeeping.
struct SweepTicket {
  bool active[kBatch] = {false};
  int ws[kBatch] = {0};  // the workspace at each column
  int n_active = 0;
  bool backward = false;
  uint64_t rows = 0;
  unsigned long long seq = 0;
};
// ws: the workspace (index into P->batch->slots and `runs`) that stands at each active column; nullptr: column c = slots[c]
int launch_sweep(pprhip_graph* P, ForaRun* runs, const bool* active, int n_active, SweepTicket* T, const int* ws = nullptr);
bool sweep_arrived(const pprhip_graph* P, const SweepTicket& T);  // collect_sweep would not wait
int collect_sweep(pprhip_graph* P, ForaRun* runs, const SweepTicket& T);

int begin_query(BatchJob& J, ForaRun& r, pprhip_graph* S, int i);  // query i of J starts on workspace S
int finish_query(BatchJob& J, ForaRun& r);  // outputs of a finished query (its slot still holds the vectors)
void share_walks_of(BatchJob& J);           // the call's terminal cache for J's seed, or none

// The sequential batch driver: kBatch resumable runs on one host thread, their dense levels served by batched sweeps on
// the handle's compute stream.  Until round 4 everything the slots did ran on that stream too, one blocking step after
// the other: the stream spent a quarter of its time in a query's sparse levels, round ends, seeds and selections - a
// few workgroups each, with a host round trip in between - while fifteen queries waited for the next sweep (kernel
// trace: 12.5 % idle + 14 % in small kernels).  Now a sweep is only LAUNCHED, and while it runs the host takes the
// slots that are not in it through their steps on a second stream (slot_stream; blocking there does not hold the
// sweep up).  What such a slot does to the shared contribution array goes to the compute stream instead (C8Scope:
// the dense prepare of its next level; the compaction back to list form), where stream order places it between two
// sweeps.  A cycle: collect the sweep in flight -> the slots that were in it say what they do next without touching the
// device (another dense level: they wait again; back to list form: the compaction is queued and the rest deferred) ->
// launch the next sweep for those who wait -> the other slots' steps (new queries, sparse levels, round ends, walk
// phases that have ended), until the sweep's counters arrive.
//
// Workspace pool (whole-graph FORA): a column of c8 is only needed between a query's first dense level and its last,
// 26 of the ~40 sweep periods a query spent in its slot on R-MAT 22 - the rest went to its first sparse levels, its
// sparse tail, the walk phase and the selection.  So there are more workspaces than columns (2 x by default,
// PPRHIP_BATCH_WORKSPACES): while sixteen queries hold the columns, the next ones are taken through their first levels
// and stand ready (kYieldColumn) when a column is let go - which happens as soon as its holder leaves a sweep without
// asking for another (the compaction that empties the column is queued first; the newcomer's prepared level lands
// behind it).  Any workspace takes any free column: at the end of a call nobody waits for a column while others idle.
constexpr int kMaxWs = 3 * kBatch;
constexpr int kDefaultWs = 2 * kBatch;

struct SlotDriver {
  pprhip_graph* P = nullptr;
  ForaRun runs[kMaxWs];
  int n_ws = kBatch;
  hipStream_t side = nullptr;  // the walk phases' stream (whole-graph FORA)
  bool walking[kMaxWs] = {false};
  bool col_marked[kMaxWs] = {false};  // col_ev of the workspace has been recorded since it began to wait for its column
  bool flying = false;
  SweepTicket ticket;
  int rr = 0;  // where the pass over the other workspaces starts (round robin: an early end must not starve anybody)
  std::function<bool(BatchJob**, int*)> next;  // the next query to start (false: none right now)
  std::function<void(BatchJob*)> done;         // a query of that job has finished
  int ready_rr = 0;         // where the search for a workspace that stands ready for a free column starts
  int cur_ws = -1;          // the workspace whose step is under way (the hook must not step it again)
  bool in_turn = false;
  KernelTimer* own_timer = g_timer_cur;  // the timer of the thread that runs the driver (turns taken from the hook restore it)
  int hook_rc = PPRHIP_OK;  // what a turn taken from inside a step's wait came to
  std::string hook_msg;
  // PPRHIP_DRIVER_PROFILE=1: host time of a turn by part, printed when the driver ends (developer switch)
  struct Prof {
    bool on = hook_env("PPRHIP_DRIVER_PROFILE") != nullptr;
    double us[6] = {0};
    unsigned long long n[6] = {0};
    std::chrono::steady_clock::time_point t;
    void start() {
      if (on) t = std::chrono::steady_clock::now();
    }
    void lap(int i) {
      if (!on) return;
      const auto now = std::chrono::steady_clock::now();
      us[i] += std::chrono::duration<double, std::micro>(now - t).count();
      n[i]++;
      t = now;
    }
    void print() const {
      if (!on) return;
      static const char* names[6] = {"collect", "owner goes on (kYield)", "owner leaves (compaction)", "newcomer takes a column", "launch", "turn from a wait"};
      for (int i = 0; i < 6; ++i)
        if (n[i]) fprintf(stderr, "[driver] %-28s %8llu x %8.1f us\n", names[i], n[i], us[i] / (double)n[i]);
    }
  } prof;

  // The driver's life: open, next / done installed, run, teardown (batch.cpp: batch_sequential; stream.cpp: stream_driver)
  int open(pprhip_graph* P_, bool pool, bool walks_beside);
  enum : int { kGoOn = PPRHIP_OK, kStop = 1 };  // after_cycle's answers besides an error code (< 0)
  int run(const char* who, const char* where, const std::function<int(int busy)>& after_cycle);
  void teardown();

 private:
  int setup(pprhip_graph* P_, bool pool, hipStream_t slots_on);
  static void on_idle(void* self);
  void release_if_idle(int w);
  int step_ws(int w, bool defer);
  int turn();
  int turn_body();
  int cycle(int* busy);
};

}  // namespace detail
}  // namespace pprhip
