// The alleles of aligned jobs: emitted, left-aligned and counted on the device, tables merged, kept alleles finished (mm_vcf.hip; the definition: mm_vcf_core.hpp).
#pragma once
#include "mm_pileup.hpp"

namespace mm {
// (w0, w1, count) triples with unique keys in ascending order of (w0, w1), in host memory
struct VcfTable { std::vector<uint64_t> w0, w1; std::vector<uint32_t> counts; };
struct VcfFinishIn {
  int64_t n; const uint64_t* w0; const uint64_t* w1; const uint32_t* counts;
  int64_t n_iv; const int32_t* iv_contig; const int64_t* iv_first; const int64_t* iv_last;
  int64_t min_count; double min_frac;
};
// the kept alleles in key order; window: mmv::WINDOW reference bytes per allele from its position on, zero beyond the contig's end
struct VcfResult { std::vector<uint64_t> w0, w1; std::vector<uint32_t> count, depth; std::vector<uint8_t> window; };
void vcf_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const PileupIn& in, VcfTable* out);
void vcf_merge_run(mm_ctx* ctx, int64_t n, const uint64_t* w0, const uint64_t* w1, const uint32_t* counts, VcfTable* out);
void vcf_finish_run(mm_ctx* ctx, const mm_seqset* reference, const VcfFinishIn& in, VcfResult* out);
}
