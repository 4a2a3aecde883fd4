// The argument rules of hnm_seqcf_fit_f32 (include/hnm.h), host code only and free of HIP so that
// a stand-alone program can run them under a sanitizer (tools/seqcf_args_check.cpp).
#pragma once
#include <stdint.h>

#include <cmath>

constexpr int SQ_MAX_N = 64;
constexpr int64_t SQ_MAX_HISTORY = 65535;
constexpr int SQ_MAX_GAP = 1024;
constexpr uint32_t SQ_GAP_ONE = 32768;  // the fixed point of the gap table: gap 1 at decay 0
constexpr int SQ_WINDOW_MAX = 16384;

// NULL when the scalar arguments are inside their ranges, else what is wrong with them.
inline const char* sq_bad_args(int N, double shrink, int64_t max_history, int max_gap,
                               int repeat_buys, int window, int64_t num_users,
                               int64_t num_items) {
  if (N < 1 || N > SQ_MAX_N) return "seqcf_fit: 1 <= N <= 64";
  if (!(shrink >= 0.0) || !std::isfinite(shrink)) return "seqcf_fit: shrink must be finite and >= 0";
  if (max_history < 1 || max_history > SQ_MAX_HISTORY) return "seqcf_fit: 1 <= max_history <= 65535";
  if (max_gap < 1 || max_gap > SQ_MAX_GAP) return "seqcf_fit: 1 <= max_gap <= 1024";
  if (repeat_buys != 0 && repeat_buys != 1) return "seqcf_fit: repeat_buys must be 0 or 1";
  if (window != 0 && (window < 64 || window > SQ_WINDOW_MAX || window % 64 != 0))
    return "seqcf_fit: window must be 0 or a multiple of 64 in [64, 16384]";
  if (num_users < 0 || num_items < 0) return "seqcf_fit: bad size";
  return nullptr;
}

// The first entry of gap_q[0, max_gap) above 2^15, or -1.
inline int sq_bad_gap_entry(const uint32_t* gap_q, int max_gap) {
  for (int g = 0; g < max_gap; ++g)
    if (gap_q[g] > SQ_GAP_ONE) return g;
  return -1;
}
