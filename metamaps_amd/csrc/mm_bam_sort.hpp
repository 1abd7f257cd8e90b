// The merge of sorted runs of BAM records into one coordinate-sorted stream of BGZF members, and its BAI index (mm_bam_sort.hip; the definitions:
// mm_bam_sort_core.hpp).
#pragma once
#include "mm_common.hpp"
#include <vector>

namespace mm {
// a run: BGZF members in the caller's memory, which hold n records back to back, ascending by (ref, pos)
struct BamSortRun {
  const uint8_t* bgzf; int64_t n;
  std::vector<int64_t> mem_off, mem_raw; std::vector<int32_t> mem_len;   // per member: where it starts in bgzf and in the inflated bytes (one more), its bytes
};
struct BamSorter {
  std::vector<int32_t> ref_len; int64_t window = 0;
  std::vector<BamSortRun> runs;
  std::vector<int32_t> ref, pos, end, run_of; std::vector<int64_t> src_off, size;   // per record in (run, index) order; src_off: in its run's inflated bytes
  bool planned = false; int64_t n = 0, stream_bytes = 0, next_window = 0;
  std::vector<int64_t> perm, out_off;                             // sorted place -> record; the sorted records' offsets in the stream (one more)
  DBuf<int64_t> d_perm, d_out_off, d_src_off; DBuf<int32_t> d_run;   // the same on the device, for the windows
  DBuf<uint8_t> d_in, d_out, tmp;
  std::vector<int32_t> member_bytes;                              // the members made so far
  std::vector<uint8_t> product;                                   // the last window's members, or the index
};
void bam_sorter_init(BamSorter& s, int32_t n_ref, const int32_t* ref_len, int64_t window_bytes);
void bam_sorter_add_run(BamSorter& s, const uint8_t* bgzf, int64_t bgzf_bytes, int64_t n_records, const int64_t* raw_off, const int32_t* ref_id, const int32_t* pos, const int32_t* end);
void bam_sorter_plan(mm_ctx* ctx, BamSorter& s);
void bam_sorter_window(mm_ctx* ctx, BamSorter& s, int64_t w);
void bam_sorter_index(mm_ctx* ctx, BamSorter& s, int64_t header_bytes);
inline int64_t bam_sorter_windows(const BamSorter& s) { return (s.stream_bytes + s.window - 1) / s.window; }
}
