// The depth profile of a set of intervals, computed on the device in memory proportional to the intervals (mm_depth.hip; the definition: mm_depth_core.hpp).
#pragma once
#include "mm_common.hpp"
#include <vector>

namespace mm {
struct DepthIn {
  int64_t n_contigs; const int64_t* contig_len;
  int64_t n_iv; const int32_t* iv_contig; const int64_t* iv_first; const int64_t* iv_last;
  int64_t window; int32_t n_thresholds; const int64_t* thresholds;
};
// the runs ordered by contig and start; contig: the contigs with an interval, ascending, with mmdp::STATS + n_thresholds counters each and their windows
// [win_off[j], win_off[j + 1]) in win_sum and win_covered
struct DepthResult {
  int32_t n_thresholds = 0;
  std::vector<int32_t> run_contig; std::vector<int64_t> run_start, run_end; std::vector<uint32_t> run_depth;
  std::vector<int32_t> contig; std::vector<int64_t> win_off{0}, stats, win_sum, win_covered;
};
void depth_profile_run(mm_ctx* ctx, const DepthIn& in, DepthResult* out);
}
