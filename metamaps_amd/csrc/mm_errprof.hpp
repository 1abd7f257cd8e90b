// The error profile of aligned jobs: counters, columns and identity keys walked on the device, per-contig rows finished there (mm_errprof.hip; the
// definition: mm_errprof_core.hpp).
#pragma once
#include "mm_jobs_dev.hpp"
#include <vector>

namespace mm {
// contig: the contigs with an alignment, ascending; stats: mmep::STATS values per listed contig, then one more row over all alignments together
struct ErrprofResult {
  std::vector<int32_t> contig; std::vector<int64_t> stats;
};
// counters[mmep::COUNTERS] is overwritten; cols[n_jobs][mmep::COLS]; ident_key[n_jobs]
void errprof_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const AlignedJobsIn& jobs, const uint8_t* use, uint64_t* counters, int32_t* cols,
                        uint64_t* ident_key);
void errprof_finish_run(mm_ctx* ctx, int64_t n_contigs, int64_t n, const uint64_t* ident_key, const int32_t* cols, ErrprofResult* out);
}
