// The identity filter of an EM problem on the device (mm_ident.hip; the definition and the pass over a read: mm_ident_core.hpp).
#pragma once
#include "mm_common.hpp"
#include "mm_ident_core.hpp"

namespace mm {
constexpr int IDENT_GROUP = 16;                                   // lanes per read of at most this many entries; longer reads take their whole wavefront
struct IdentIn { int64_t n_reads; const int64_t* read_off; const int32_t* taxon; const double* ident; const int64_t* best; int32_t n_taxa; double thr; };
struct IdentOut {
  double* sorted_max; int64_t* n_with_entries; int64_t* n_le; int64_t* taxon_reads; double* taxon_median; uint8_t* taxon_removed; uint8_t* read_removed;
  int64_t* read_src; int64_t* entry_src; int64_t* read_off_out; int64_t* n_reads_out; int64_t* n_entries_out;   // the filtered problem: all five, or all null
};
void ident_filter_run(mm_ctx* ctx, const IdentIn& in, const IdentOut& out);
}
