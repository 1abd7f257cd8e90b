// Gene-level analysis of best mappings on the device (mm_gene.hip; the definition and the stabbing query: mm_gene_core.hpp).
#pragma once
#include "mm_common.hpp"
#include "mm_gene_core.hpp"

namespace mm {
constexpr int GENE_LANE_SPAN = 64;                                // a mapping with more candidate genes than this is walked by its whole wavefront
constexpr int64_t GENE_PAIR_BUDGET = (int64_t)1 << 26;            // (mapping, gene) pairs, feature keys and median keys per tile (MM_GENE_PAIR_BUDGET)
struct GeneIn {
  int32_t n_contigs; const int64_t* contig_gene_off; const int32_t* gene_start; const int32_t* gene_stop; const int32_t* gene_group; int32_t n_groups;
  const int64_t* group_feat_off; const int32_t* group_feat; int32_t n_feats;
  int64_t n_maps; const int32_t* map_contig; const int32_t* map_start; const int32_t* map_stop; const double* map_ident;
};
// group_reads[n_groups], group_median[n_groups] (NaN where group_reads is 0), feat_reads[n_feats] (may be null), maps_on_annotated (may be null)
void gene_overlap_run(mm_ctx* ctx, const GeneIn& in, int64_t* group_reads, double* group_median, int64_t* feat_reads, int64_t* maps_on_annotated);
}
