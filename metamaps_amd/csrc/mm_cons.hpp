// The consensus of a group of contigs, built on the device from a merged allele table and the alignments' intervals (mm_cons.hip; the definition: mm_cons_core.hpp).
#pragma once
#include "mm_keytable.hpp"

namespace mm {
// a group [contig_lo, contig_hi) of the reference, its rows and intervals (table.min_count is not read: a candidate needs one read; table.min_frac is F)
struct ConsIn { int32_t contig_lo, contig_hi; FinishIn table; int64_t min_depth; double min_called; int32_t line_width; };
// contig: the group's contigs with an interval, ascending, with mmc::STATS counters each; written: those of them whose text is there, text_off[j] the start of
// written[j]'s wrapped lines in text, text_off[written.size()] the bytes of text
struct ConsResult { std::vector<int32_t> contig, written; std::vector<int64_t> stats, text_off; std::vector<uint8_t> text; };
void consensus_run(mm_ctx* ctx, const mm_seqset* reference, const ConsIn& in, ConsResult* out);
}
