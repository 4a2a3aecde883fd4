// The host-side argument rules of hnm_seqcf_fit_f32 (csrc/seqcf_args.h) as a stand-alone CPU
// program, so that they can run under a sanitizer without a GPU and without Python:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I hnm_recommendation_amd/csrc tools/seqcf_args_check.cpp -o seqcf_args_check
//   ./seqcf_args_check
//
// Exit status 0 and "seqcf_args_check: ok" when every case gives the documented answer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "seqcf_args.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n", what);
    ++failures;
  }
}

// The accepted call of every case below, one argument replaced at a time.
static const char* args(int N = 64, double shrink = 0.0, int64_t max_history = 65535,
                        int max_gap = 28, int repeat = 0, int window = 0, int64_t U = 10,
                        int64_t I = 10) {
  return sq_bad_args(N, shrink, max_history, max_gap, repeat, window, U, I);
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double inf = std::numeric_limits<double>::infinity();
  expect(args() == nullptr, "the defaults are accepted");
  expect(args(1) == nullptr && args(0) != nullptr && args(65) != nullptr && args(-3) != nullptr,
         "1 <= N <= 64");
  expect(args(64, 2.5) == nullptr && args(64, -0.0) == nullptr, "shrink >= 0");
  expect(args(64, -1e-9) && args(64, nan) && args(64, inf) && args(64, -inf), "shrink finite");
  expect(args(64, 0, 1) == nullptr && args(64, 0, 0) && args(64, 0, 65536) && args(64, 0, -1) &&
             args(64, 0, std::numeric_limits<int64_t>::max()),
         "1 <= max_history <= 65535");
  expect(args(64, 0, 9, 1) == nullptr && args(64, 0, 9, 1024) == nullptr && args(64, 0, 9, 0) &&
             args(64, 0, 9, 1025) && args(64, 0, 9, std::numeric_limits<int>::min()),
         "1 <= max_gap <= 1024");
  expect(args(64, 0, 9, 7, 1) == nullptr && args(64, 0, 9, 7, 2) && args(64, 0, 9, 7, -1),
         "repeat_buys is 0 or 1");
  for (int w : {64, 128, 8192, 16384}) expect(args(64, 0, 9, 7, 0, w) == nullptr, "window ok");
  for (int w : {1, 32, 63, 100, 16384 + 64, -64, std::numeric_limits<int>::max()})
    expect(args(64, 0, 9, 7, 0, w) != nullptr, "window refused");
  expect(args(64, 0, 9, 7, 0, 0, 0, 0) == nullptr && args(64, 0, 9, 7, 0, 0, -1, 5) &&
             args(64, 0, 9, 7, 0, 0, 5, -1),
         "sizes >= 0");

  // the gap table: exactly max_gap entries are read (a heap block of that size: one entry more
  // would be an out-of-bounds read under the sanitizer)
  for (int max_gap : {1, 2, 28, 1024}) {
    std::vector<uint32_t> q((size_t)max_gap, SQ_GAP_ONE);
    expect(sq_bad_gap_entry(q.data(), max_gap) == -1, "a table of 32768 is accepted");
    q[(size_t)max_gap - 1] = SQ_GAP_ONE + 1;
    expect(sq_bad_gap_entry(q.data(), max_gap) == max_gap - 1, "the last entry is checked");
    q[0] = 0xffffffffu;
    expect(sq_bad_gap_entry(q.data(), max_gap) == 0, "the first bad entry is named");
    q[0] = 0;
    q[(size_t)max_gap - 1] = 0;
    expect(sq_bad_gap_entry(q.data(), max_gap) == -1, "zeros are accepted");
  }
  if (failures) return EXIT_FAILURE;
  std::puts("seqcf_args_check: ok");
  return EXIT_SUCCESS;
}
