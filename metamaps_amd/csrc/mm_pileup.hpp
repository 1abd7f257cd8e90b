// The pileup of aligned jobs: events counted on the device, tables merged, sites and coverage finished (mm_pileup.hip; the definition: mm_pileup_core.hpp).
#pragma once
#include "mm_common.hpp"
#include <vector>

namespace mm {
// the caller's arrays, as mm_pileup_events takes them
struct PileupIn {
  int64_t n_jobs; const int32_t* read; const int32_t* strand; const int32_t* contig; const int32_t* dist; const int64_t* first;
  const int64_t* op_off; const uint32_t* ops; const uint8_t* use;
};
// (key, count) pairs with unique keys in ascending order, in host memory
struct PileupTable { std::vector<uint64_t> keys; std::vector<uint32_t> counts; };
struct PileupFinishIn {
  int64_t n; const uint64_t* keys; const uint32_t* counts;
  int64_t n_iv; const int32_t* iv_contig; const int64_t* iv_first; const int64_t* iv_last;
  int64_t min_count; double min_frac;
};
// the kept sites in key order, and the coverage of every contig of the reference
struct PileupResult {
  std::vector<uint64_t> key; std::vector<uint32_t> count, depth; std::vector<uint8_t> ref_byte;
  std::vector<int64_t> alignments, covered, sum_depth;
};
void pileup_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const PileupIn& in, PileupTable* out);
void pileup_merge_run(mm_ctx* ctx, int64_t n, const uint64_t* keys, const uint32_t* counts, PileupTable* out);
void pileup_finish_run(mm_ctx* ctx, const mm_seqset* reference, const PileupFinishIn& in, PileupResult* out);
}
