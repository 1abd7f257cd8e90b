// The pileup of aligned jobs: events counted on the device, tables merged, sites and coverage finished (mm_pileup.hip; the definition: mm_pileup_core.hpp).
#pragma once
#include "mm_jobs_dev.hpp"
#include "mm_keytable.hpp"

namespace mm {
// the kept sites in key order (w0: the keys), and the coverage of every contig of the reference
struct PileupResult : KeptRows {
  std::vector<uint8_t> ref_byte;
  std::vector<int64_t> alignments, covered, sum_depth;
};
// use: one byte per job beside the aligned jobs (mm_jobs_dev.hpp); the events are mm_events.hpp's pipeline with the format's kernels
void pileup_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const AlignedJobsIn& jobs, const uint8_t* use, int32_t min_base_quality, KeyTable* out);
void pileup_finish_run(mm_ctx* ctx, const mm_seqset* reference, const FinishIn& in, PileupResult* out);
}
