// The alleles of aligned jobs: emitted, left-aligned and counted on the device, tables merged, kept alleles finished (mm_vcf.hip; the definition: mm_vcf_core.hpp).
#pragma once
#include "mm_jobs_dev.hpp"
#include "mm_keytable.hpp"

namespace mm {
// the kept alleles in key order; window: mmv::WINDOW reference bytes per allele from its position on, zero beyond the contig's end
struct VcfResult : KeptRows { std::vector<uint64_t> w1; std::vector<uint8_t> window; };
// use: as mm_pileup.hpp's
void vcf_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const AlignedJobsIn& jobs, const uint8_t* use, int32_t min_base_quality, KeyTable* out);
void vcf_finish_run(mm_ctx* ctx, const mm_seqset* reference, const FinishIn& in, VcfResult* out);
}
