// Host-side check of md_gather_row / md_kahan_add (csrc/md_gather.h), built with the address and undefined-behaviour sanitizers
// by tests/test_cpu_csr_host.py and run as a child process.  No kernel is instantiated and no GPU is touched.  Every array is a
// heap block of exactly its size, so a read the guards should have stopped is a sanitizer report.
#include <cstdio>
#include <vector>

#include "md_gather.h"

static int failures = 0;

#define EXPECT(cond, ...)                  \
  do {                                     \
    if (!(cond)) {                         \
      ++failures;                          \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);            \
      std::printf("\n");                   \
    }                                      \
  } while (0)

// src[code][c] = 7 code + 3 c - 20: small integers of both signs, so fp32 sums are exact in any order and for both sum kinds
static float src_value(int code, int c) { return (float)(7 * code + 3 * c - 20); }

template <int W>
static std::vector<float> make_src(int n_codes) {
  std::vector<float> src((size_t)n_codes * W);
  for (int code = 0; code < n_codes; ++code)
    for (int c = 0; c < W; ++c) src[(size_t)code * W + c] = src_value(code, c);
  return src;
}

// the CSR of dest (stable: ascending code inside a row), built by counting
static void make_csr(const std::vector<int>& dest, int rows, std::vector<int32_t>& ptr, std::vector<int32_t>& order) {
  ptr.assign(rows + 1, 0);
  order.clear();
  for (int r = 0; r < rows; ++r) {
    for (int code = 0; code < (int)dest.size(); ++code)
      if (dest[code] == r) order.push_back(code);
    ptr[r + 1] = (int32_t)order.size();
  }
}

template <int W, bool KAHAN>
static void check_sums() {
  // rows 0, 3 and 6 are empty (start, middle, end); row 2 holds five codes, rows 1, 4 and 5 two each
  const std::vector<int> dest = {2, 1, 2, 5, 4, 2, 1, 5, 2, 4, 2};
  const int rows = 7, n_codes = (int)dest.size();
  std::vector<int32_t> ptr, order;
  make_csr(dest, rows, ptr, order);
  const std::vector<float> src = make_src<W>(n_codes);
  for (int r = 0; r < rows; ++r) {
    float acc[W];
    for (int c = 0; c < W; ++c) acc[c] = -1.f;               // the row loop must overwrite, not accumulate into, acc
    md_gather_row<W, KAHAN>(src.data(), ptr.data(), order.data(), r, n_codes, acc);
    for (int c = 0; c < W; ++c) {
      long want = 0;
      for (int code = 0; code < n_codes; ++code)
        if (dest[code] == r) want += 7 * code + 3 * c - 20;
      EXPECT(acc[c] == (float)want, "W=%d kahan=%d row=%d c=%d: got %g, want %ld", W, (int)KAHAN, r, c, (double)acc[c], want);
    }
  }
}

// A broken CSR: nothing outside the arrays may be read, and what is inside still counts.
template <int W, bool KAHAN>
static void check_guards() {
  const int n_codes = 4;
  const std::vector<float> src = make_src<W>(n_codes);
  // row 0: ptr[1] = 9 runs past n_codes: positions 0..3 are summed, then the loop stops.
  //        order holds a negative code (skipped), code 4 >= n_codes (skipped), code 1 and code 3.
  // row 1: ptr[1] = 9 .. ptr[2] = 12 starts outside: nothing.
  // row 2: ptr[2] = 12 .. ptr[3] = 2, an empty span.
  // row 3: ptr[3] = -2 .. ptr[4] = 3 starts negative: nothing.
  const std::vector<int32_t> ptr = {0, 9, 12, -2, 3};
  const std::vector<int32_t> order = {-1, 4, 1, 3};
  for (int r = 0; r < 4; ++r) {
    float acc[W];
    md_gather_row<W, KAHAN>(src.data(), ptr.data(), order.data(), r, n_codes, acc);
    for (int c = 0; c < W; ++c) {
      const float want = r == 0 ? src_value(1, c) + src_value(3, c) : 0.f;
      EXPECT(acc[c] == want, "guards W=%d kahan=%d row=%d c=%d: got %g, want %g", W, (int)KAHAN, r, c, (double)acc[c], (double)want);
    }
  }
}

// Where the two kinds differ.  fp32 near 2^24 = 16777216 has a spacing of 2, ties round to the even significand.
//   terms: 16777216, 1, 1, 1, 1                                        exact sum 16777220
//   plain: 16777216 + 1 = 16777217 -> tie -> 16777216, four times: 16777216.
//   Kahan: sum = 16777216, lost = 0
//     x = 1: y = 1, t = 16777217 -> 16777216, lost = (t - sum) - y = -1, sum = 16777216
//     x = 1: y = 1 - (-1) = 2, t = 16777218 (exact), lost = 2 - 2 = 0, sum = 16777218
//     x = 1: y = 1, t = 16777219 -> tie between ...218 (odd significand) and ...220 (even) -> 16777220, lost = 2 - 1 = 1
//     x = 1: y = 1 - 1 = 0, t = 16777220, lost = 0: 16777220.
// The terms 1e8, 1, 1, 1, 1, -1e8 (spacing 8 near 1e8) do NOT separate the kinds, and pin why: every 1 is dropped by both, Kahan
// carries lost = -4 into the last step, where y = -1e8 + 4 is the tie between -99999992 and -1e8 and rounds to -1e8 (even), so the
// compensation is rounded away: plain 0, Kahan 0 (exact sum 4).  One more 1 gets through: 1e8, 1 x 5, -1e8 gives
//     5th x = 1: y = 1 + 4 = 5, t = 1e8 + 5 -> 1e8 + 8, lost = 8 - 5 = 3; x = -1e8: y = -1e8 - 3 -> -1e8, t = 8, lost = 0
// plain 0, Kahan 8 (exact sum 5).
static void check_kahan() {
  struct Case { std::vector<float> terms; float plain, kahan; };
  const Case cases[] = {
      {{16777216.f, 1.f, 1.f, 1.f, 1.f}, 16777216.f, 16777220.f},
      {{1e8f, 1.f, 1.f, 1.f, 1.f, -1e8f}, 0.f, 0.f},
      {{1e8f, 1.f, 1.f, 1.f, 1.f, 1.f, -1e8f}, 0.f, 8.f},
  };
  for (const Case& k : cases) {
    const int n = (int)k.terms.size();
    const std::vector<int32_t> ptr = {0, n};
    std::vector<int32_t> order(n);
    for (int j = 0; j < n; ++j) order[j] = j;
    float plain[1], kahan[1];
    md_gather_row<1, false>(k.terms.data(), ptr.data(), order.data(), 0, n, plain);
    md_gather_row<1, true>(k.terms.data(), ptr.data(), order.data(), 0, n, kahan);
    EXPECT(plain[0] == k.plain, "plain sum of %d terms: got %.1f, want %.1f", n, (double)plain[0], (double)k.plain);
    EXPECT(kahan[0] == k.kahan, "Kahan sum of %d terms: got %.1f, want %.1f", n, (double)kahan[0], (double)k.kahan);
    float sum = 0.f, lost = 0.f;                             // md_kahan_add on its own is the same step
    for (float x : k.terms) md_kahan_add(sum, lost, x);
    EXPECT(sum == k.kahan, "md_kahan_add over %d terms: got %.1f, want %.1f", n, (double)sum, (double)k.kahan);
  }
}

template <int W>
static void check_width() {
  check_sums<W, false>();
  check_sums<W, true>();
  check_guards<W, false>();
  check_guards<W, true>();
}

int main() {
  check_width<1>();
  check_width<3>();
  check_width<8>();
  check_kahan();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("gather_row: ok\n");
  return 0;
}
