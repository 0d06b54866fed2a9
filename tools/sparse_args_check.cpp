// sparse_args_check.cpp — the device-free half of the sparse getters (csrc/sparse_args.hpp: argument checks, cap and
// growth arithmetic) as a stand-alone program, for a sanitizer build on a machine without a GPU:
//   make -C personalized-pagerank-algorithms-on-neo4j_amd sparse-args-check
// Exit status 0 and "sparse_args_check: ok" when every case holds.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "../personalized-pagerank-algorithms-on-neo4j_amd/csrc/sparse_args.hpp"

static std::string g_error;
namespace pprhip {
void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_error = buf;
}
}  // namespace pprhip

using pprhip::detail::sparse_check_args;
using pprhip::detail::sparse_grown;
using pprhip::detail::sparse_take;

static int g_failed = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      ++g_failed;                                                           \
      fprintf(stderr, "line %d: %s (last error: %s)\n", __LINE__, #cond, g_error.c_str()); \
    }                                                                       \
  } while (0)

static bool says(const char* a, const char* b = "") {
  return g_error.find(a) != std::string::npos && g_error.find(b) != std::string::npos;
}

int main() {
  const char* fns[] = {"pprhip_get_reserve_sparse", "pprhip_get_residue_sparse", "pprhip_results_fetch_sparse",
                       "pprhip_results_fetch_sparse_all"};
  int32_t ids[4] = {0};
  double vals[4] = {0};
  uint64_t count = 0;
  const double inf = std::numeric_limits<double>::infinity();
  const double bad_thr[] = {-1e-300, -5e-324, std::nan(""), inf, -inf, -1.0};
  const double good_thr[] = {0.0, -0.0, 5e-324, 1e-300, 1.0, std::numeric_limits<double>::max()};
  for (const char* fn : fns) {
    for (double t : bad_thr) {
      EXPECT(sparse_check_args(fn, t, 0, ids, vals, 4, &count, true) == PPRHIP_ERR_INVALID);
      EXPECT(says(fn, "threshold = "));
    }
    for (int o : {-1, 2, 3, std::numeric_limits<int>::min(), std::numeric_limits<int>::max()}) {
      EXPECT(sparse_check_args(fn, 0.0, o, ids, vals, 4, &count, true) == PPRHIP_ERR_INVALID);
      EXPECT(says(fn, "order = "));
    }
    EXPECT(sparse_check_args(fn, 0.0, 0, ids, vals, 4, nullptr, true) == PPRHIP_ERR_INVALID && says(fn, "count"));
    EXPECT(sparse_check_args(fn, 0.0, 0, ids, vals, 4, &count, false) == PPRHIP_ERR_INVALID && says(fn, "offsets_out"));
    EXPECT(sparse_check_args(fn, 0.0, 1, ids, nullptr, 0, &count, true) == PPRHIP_ERR_INVALID && says(fn, "cap = 0"));
    EXPECT(sparse_check_args(fn, 0.0, 1, nullptr, vals, 0, &count, true) == PPRHIP_ERR_INVALID && says(fn, "cap = 0"));
    for (double t : good_thr)
      for (int o : {0, 1}) {
        EXPECT(sparse_check_args(fn, t, o, nullptr, nullptr, 0, &count, true) == PPRHIP_OK);
        EXPECT(sparse_check_args(fn, t, o, ids, vals, 4, &count, true) == PPRHIP_OK);
        EXPECT(sparse_check_args(fn, t, o, ids, nullptr, 1, &count, true) == PPRHIP_OK);
        EXPECT(sparse_check_args(fn, t, o, nullptr, nullptr, ~0ull, &count, true) == PPRHIP_OK);
      }
  }
  // the entries a call writes: min(cap, total), none without a buffer
  const uint64_t big = ~0ull;
  EXPECT(sparse_take(0, 0, false) == 0 && sparse_take(0, 9, false) == 0 && sparse_take(9, 9, false) == 0);
  EXPECT(sparse_take(1, 0, true) == 0 && sparse_take(1, 9, true) == 1 && sparse_take(8, 9, true) == 8);
  EXPECT(sparse_take(9, 9, true) == 9 && sparse_take(14, 9, true) == 9 && sparse_take(big, 9, true) == 9);
  EXPECT(sparse_take(9, big, true) == 9 && sparse_take(big, big, true) == big);
  // growth: never below the need, never wrapping
  for (size_t need : {(size_t)0, (size_t)1, (size_t)63, (size_t)1 << 20, (size_t)1 << 40, SIZE_MAX / 2, SIZE_MAX - 64,
                      SIZE_MAX - 1, SIZE_MAX}) {
    EXPECT(sparse_grown(need) >= need);
    if (need < SIZE_MAX / 2) EXPECT(sparse_grown(need) == need + need / 8 + 64);
  }
  EXPECT(sparse_grown(SIZE_MAX) == SIZE_MAX && sparse_grown(SIZE_MAX - 10) == SIZE_MAX);
  // a cap that ends in the middle of a CSR row: rows of 3, 0, 5 entries, cap 5 -> row 2 gets its first two
  {
    const uint64_t offs[] = {0, 3, 3, 8};
    const uint64_t take = sparse_take(5, offs[3], true);
    uint64_t per_row[3];
    for (int i = 0; i < 3; ++i) {
      const uint64_t lo = offs[i] < take ? offs[i] : take, hi = offs[i + 1] < take ? offs[i + 1] : take;
      per_row[i] = hi - lo;
    }
    EXPECT(per_row[0] == 3 && per_row[1] == 0 && per_row[2] == 2);
  }
  if (g_failed) {
    fprintf(stderr, "sparse_args_check: %d failed\n", g_failed);
    return 1;
  }
  printf("sparse_args_check: ok\n");
  return 0;
}
