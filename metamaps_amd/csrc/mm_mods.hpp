// Base modifications: the (who, prob) plane of a read set made from its reads' MM/ML groups, the calls of aligned jobs counted per reference
// position, tables merged, rows finished (mm_mods.hip; the definition: mm_mods_core.hpp).
#pragma once
#include "mm_jobs_dev.hpp"
#include "mm_keytable.hpp"
#include "mm_mods_core.hpp"
#include "mm_seq.hpp"

namespace mm {
// the rows in the order contig, position, + before -, the asked codes' order
struct ModResult { std::vector<uint64_t> site, n_mod, n_canonical, n_other, n_fail; };
// What mm_mod_finish and mm_mod_motifs check on the host before anything is launched, stated once: the reference (uploaded, on ctx's device, at most 2^28
// contigs), the codes' bases, min_coverage, and the merged table (keys ascending and unique, each naming a position of the reference and a class of the asked
// codes).  `w` starts every message ("mm_mod_finish: ").  Returns the codes' bases for the kernels.
mmd::CodeBases mod_table_checks(const std::string& w, mm_ctx* ctx, const mm_seqset* reference, int64_t n, const uint64_t* keys, int32_t n_codes, const uint8_t* code_base,
                                int64_t min_coverage);
void mod_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const AlignedJobsIn& jobs, const uint8_t* use, int32_t min_ml, KeyTable* out);
void mod_finish_run(mm_ctx* ctx, const mm_seqset* reference, int64_t n, const uint64_t* keys, const uint32_t* counts, int32_t n_codes, const uint8_t* code_base, int64_t min_coverage,
                    ModResult* out);
}
