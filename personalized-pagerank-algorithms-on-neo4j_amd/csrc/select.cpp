// select.cpp — the top-k selection driver (Algo_Util.kth_ppr + retrieveTopK): launches the radix select of
// kernels_select.hip, reads its header and candidates back (device_io.cpp: fetch_*) and orders them on the host.
// Callers: pprhip_topk_select (engine.cpp) and the top-k rounds of fora.cpp.
#include <algorithm>
#include <cstring>

#include "engine_internal.hpp"

using namespace pprhip;
using namespace pprhip::detail;

namespace pprhip {
namespace detail {

// ------------------------------------------------------------------ top-k selection driver
struct IdVal {
  int32_t id;
  double val;
};

// candidates (all entries >= the lower edge of the bin that holds the k-th largest) -> the reference's answer
static void finish_select(std::vector<IdVal>& cand, bool have, int k, int32_t* ids_out, double* vals_out, int cap,
                          int* n_out, double* kth_out, bool* have_kth, pprhip_stats_t& st) {
  std::sort(cand.begin(), cand.end(), [](const IdVal& a, const IdVal& b) {
    if (a.val != b.val) return a.val > b.val;
    return a.id < b.id;
  });
  size_t n_sel = cand.size();
  double kth = 0.0;
  if (have) {
    kth = cand[(size_t)k - 1].val;
    n_sel = 0;
    while (n_sel < cand.size() && cand[n_sel].val >= kth) ++n_sel;
  }
  for (size_t i = 0; i < n_sel && (int)i < cap; ++i) {
    if (ids_out) ids_out[i] = cand[i].id;
    if (vals_out) vals_out[i] = cand[i].val;
  }
  *n_out = (int)n_sel;
  *have_kth = have;
  if (kth_out) *kth_out = kth;
  st.kth_value = kth;
}

// The multi-pass form: the host reads every histogram and refines the prefix until few enough candidates are left
// (needed when more than sel_cap entries share the leading 12 bits of the k-th largest).
static int select_topk_passes(pprhip_graph* g, const double* x, int k, int32_t* ids_out, double* vals_out, int cap,
                              int* n_out, double* kth_out, bool* have_kth, pprhip_stats_t& st) {
  std::vector<uint32_t> hist(4096);
  unsigned long long prefix = 0;
  int pbits = 0;
  uint64_t k_rem = (uint64_t)k;
  uint64_t above = 0;  // entries in bins above the chosen prefix
  uint64_t total = 0;
  bool have = true;
  unsigned long long lower_bits = 1ull;  // smallest positive pattern: "everything"
  uint64_t expected = ~0ull;              // candidates the gather will find, known from the histograms
  for (int pass = 0; pbits < 64; ++pass) {
    const int dbits = std::min(12, 64 - pbits);
    PPRHIP_TRY(launch_select_hist(g, x, act_n(g), prefix, pbits, dbits, pass == 0));
    PPRHIP_CHECK_HIP(hipMemcpyAsync(hist.data(), g->hist, sizeof(uint32_t) * (1u << dbits), hipMemcpyDeviceToHost,
                                    g->stream));
    PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    st.select_passes++;
    st.select_bytes += 8ull * g->gr->n;
    if (pass == 0) {
      for (uint32_t b = 0; b < (1u << dbits); ++b) total += hist[b];
      if (total == 0) {
        PPRHIP_CHECK_HIP(hipMemsetAsync(g->hist, 0, sizeof(uint32_t) * 4096, g->stream));
        *n_out = 0;
        *have_kth = false;
        if (kth_out) *kth_out = 0.0;
        return PPRHIP_OK;
      }
      if ((uint64_t)k > total) {  // kth_ppr returns null: everything is kept (Fora_Topk.java:187-191)
        have = false;
        expected = total;
        break;
      }
    }
    uint64_t cum = 0;
    int chosen = -1;
    for (int b = (1 << dbits) - 1; b >= 0; --b) {
      if (cum + hist[b] >= k_rem) {
        chosen = b;
        break;
      }
      cum += hist[b];
    }
    if (chosen < 0) {
      set_error("select_topk: histogram inconsistent (k_rem=%llu)", (unsigned long long)k_rem);
      return PPRHIP_ERR_STATE;
    }
    above += cum;
    k_rem -= cum;
    prefix = (prefix << dbits) | (unsigned long long)chosen;
    pbits += dbits;
    lower_bits = pbits < 64 ? (prefix << (64 - pbits)) : prefix;
    expected = above + hist[chosen];
    if (expected <= g->sel_cap) break;  // few enough candidates: finish on the host
  }
  PPRHIP_TRY(launch_select_gather(g, x, act_n(g), have ? lower_bits : 1ull, false));
  // the histograms already say how many candidates there are: the count and the records come back in ONE copy
  const bool prefetched = expected > 0 && expected <= g->sel_cap;
  const size_t want = prefetched ? (size_t)expected : 0;
  std::vector<char> blob(kSelHeader + sizeof(SelRec) * want);
  PPRHIP_TRY(fetch_small(g, g->sel_blob, blob.data(), blob.size()));
  st.select_bytes += 8ull * g->gr->n;
  uint64_t cnt = 0;
  std::memcpy(&cnt, blob.data(), 8);
  std::vector<IdVal> cand;
  auto take_recs = [&](const char* p, uint64_t c) {
    cand.resize(c);
    const SelRec* r = reinterpret_cast<const SelRec*>(p);
    for (uint64_t i = 0; i < c; ++i) cand[i] = {g->gr->h_new2old[r[i].id], r[i].val};
  };
  if (prefetched && cnt == expected) {
    take_recs(blob.data() + kSelHeader, cnt);
  } else if (cnt <= g->sel_cap) {
    std::vector<char> more(sizeof(SelRec) * cnt);
    if (cnt) {
      PPRHIP_CHECK_HIP(hipMemcpyAsync(more.data(), g->sel_blob + kSelHeader, more.size(), hipMemcpyDeviceToHost, g->stream));
      PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    }
    take_recs(more.data(), cnt);
  } else {
    // more ties at the k-th value than the candidate buffer holds: finish on the whole vector
    std::vector<double> all(g->gr->n);
    PPRHIP_CHECK_HIP(hipMemcpyAsync(all.data(), x, sizeof(double) * g->gr->n, hipMemcpyDeviceToHost, g->stream));
    PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    const double lb = [&] { double d; std::memcpy(&d, &lower_bits, 8); return d; }();
    for (uint32_t i = 0; i < g->gr->n; ++i)
      if (all[i] > 0.0 && (!have || all[i] >= lb)) cand.push_back({g->gr->h_new2old[i], all[i]});
  }
  finish_select(cand, have, k, ids_out, vals_out, cap, n_out, kth_out, have_kth, st);
  return PPRHIP_OK;
}

// k-th largest and the entries >= it (Algo_Util.kth_ppr + retrieveTopK).  One histogram pass over the 12 leading bits,
// the bin of the k-th largest chosen on the device, the gather of everything from that bin's lower edge up, and ONE
// read-back (header + the first kPre records; the candidates are then ordered on the host, values descending, ids
// ascending).  Only when more candidates share those 12 bits than the buffer holds the multi-pass form takes over.
// The selection in two halves, so that a caller can queue other work between launching it and waiting for it.
constexpr size_t kSelPre = 2048;
int select_launch(pprhip_graph* g, const double* x, int k, unsigned long long* seq_out, bool with_plan_sum) {
  poll_idle(g);
  {
    SetupScope setup(g);
    PPRHIP_TRY(launch_select_hist(g, x, act_n(g), 0ull, 0, 12, true));
    PPRHIP_TRY(launch_select_choose(g, (unsigned long long)k));
    // with_plan_sum: the residue sum of the round whose plan ran last travels in the header (DevCounters::plan_sum)
    PPRHIP_TRY(launch_select_gather(g, x, act_n(g), 0ull, false, true,
                                    with_plan_sum ? &g->ctr->plan_sum[g->mc_last_plan % 3u] : nullptr));
  }
  return fetch_begin(g, g->sel_blob, kSelHeader + sizeof(SelRec) * kSelPre, seq_out);
}

int select_topk(pprhip_graph* g, const double* x, int k, int32_t* ids_out, double* vals_out, int cap, int* n_out,
                double* kth_out, bool* have_kth, pprhip_stats_t& st, bool with_plan_sum) {
  unsigned long long seq = 0;
  PPRHIP_TRY(select_launch(g, x, k, &seq, with_plan_sum));
  return select_finish(g, seq, x, k, ids_out, vals_out, cap, n_out, kth_out, have_kth, st);
}

int select_finish(pprhip_graph* g, unsigned long long seq, const double* x, int k, int32_t* ids_out, double* vals_out,
                  int cap, int* n_out, double* kth_out, bool* have_kth, pprhip_stats_t& st) {
  constexpr size_t kPre = kSelPre;
  std::vector<char> blob(kSelHeader + sizeof(SelRec) * kPre);
  PPRHIP_TRY(fetch_end(g, seq, g->sel_blob, blob.data(), blob.size()));
  st.select_passes++;
  st.select_bytes += 16ull * act_n(g);
  unsigned long long hdr[6];
  std::memcpy(hdr, blob.data(), sizeof hdr);
  const uint64_t cnt = hdr[0], expected = hdr[2], total = hdr[3];
  const bool have = hdr[4] != 0;
  std::memcpy(&g->sel_plan_sum, &hdr[5], sizeof(double));  // (meaningful after select_launch(..., with_plan_sum))
  if (total == 0) {
    *n_out = 0;
    *have_kth = false;
    if (kth_out) *kth_out = 0.0;
    return PPRHIP_OK;
  }
  if (expected > g->sel_cap || cnt != expected)  // too many share the leading bits (or the header is not what it should be)
    return select_topk_passes(g, x, k, ids_out, vals_out, cap, n_out, kth_out, have_kth, st);
  std::vector<IdVal> cand(cnt);
  const std::vector<int32_t>& n2o = g->gr->h_new2old;
  if (cnt <= kPre) {
    const SelRec* r = reinterpret_cast<const SelRec*>(blob.data() + kSelHeader);
    for (uint64_t i = 0; i < cnt; ++i) cand[i] = {n2o[r[i].id], r[i].val};
  } else {
    std::vector<SelRec> more(cnt);
    PPRHIP_CHECK_HIP(hipMemcpyAsync(more.data(), g->sel_blob + kSelHeader, sizeof(SelRec) * cnt, hipMemcpyDeviceToHost, g->stream));
    PPRHIP_CHECK_HIP(hipStreamSynchronize(g->stream));
    for (uint64_t i = 0; i < cnt; ++i) cand[i] = {n2o[more[i].id], more[i].val};
  }
  finish_select(cand, have, k, ids_out, vals_out, cap, n_out, kth_out, have_kth, st);
  return PPRHIP_OK;
}

}  // namespace detail
}  // namespace pprhip
