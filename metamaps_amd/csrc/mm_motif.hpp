// Methylation per sequence motif over a group of consecutive contigs (mm_mod_motifs; mm_motif.hip; the definition: mm_motif_core.hpp).
#pragma once
#include "mm_motif_core.hpp"
#include "mm_seq.hpp"

namespace mm {
struct MotifIn {
  int32_t contig_lo, contig_hi; int64_t n; const uint64_t* keys; const uint32_t* counts; int32_t n_codes; const uint8_t* code_base;
  int32_t n_motifs; const int32_t* motif_off; const uint8_t* motif_mask; const int32_t* motif_pos; int64_t min_coverage; double min_frac; int32_t combine;
};
// rows in the order contig, position, + before -, motif, code; the summary in the order listed contig, motif, applicable code, mmt::SUMS sums each
struct MotifResult {
  std::vector<uint64_t> site, n_mod, n_canonical, n_other, n_fail; std::vector<int32_t> motif, code;
  std::vector<int32_t> s_contig, s_motif, s_code; std::vector<int64_t> sums;
};
void mod_motifs_run(mm_ctx* ctx, const mm_seqset* reference, const MotifIn& in, MotifResult* out);
}
