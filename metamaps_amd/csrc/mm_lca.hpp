// Confidence-thresholded LCA assignment of the reads of an EM problem on the device (mm_lca.hip; the definition and the per-read routine: mm_lca_core.hpp).
#pragma once
#include "mm_em.hpp"
#include "mm_lca_core.hpp"

namespace mm {
constexpr int LCA_GROUP = 16;                                     // lanes of a short read's group: reads of up to 16 entries, four to a wavefront, one lane per entry
constexpr int LCA_LDS_NODES = 4096;                               // trees up to this size are copied into LDS (12 bytes per node: 48 KiB at most)
// posteriors of `f` (as mm_em_posteriors), then node_out[n_reads], mass_out[n_reads] (may be null), direct_out[n_nodes] (may be null)
void lca_run(mm_em* E, const double* f, int32_t n_nodes, const int32_t* parent, const int32_t* taxon_node, double tau,
             int32_t* node_out, double* mass_out, int64_t* direct_out);
}
