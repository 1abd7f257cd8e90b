// FASTQ / FASTA records of selected reads of a set, written and deflated on the device (mm_reads_out.hip; the record: mm_reads_out_core.hpp).
#pragma once
#include "mm_common.hpp"
#include "mm_codec.hpp"                                            // (bgzf_deflate_resident: BGZF members of input that lies on the device)
#include <vector>

namespace mm {
// the caller's arrays as mm_reads_encode takes them: record i is read read[i] of the set under the name names[name_off[i], name_off[i + 1])
struct ReadsSelection { int64_t n; const int32_t* read; const int64_t* name_off; const char* names; };
// the members of every group back to back, in host memory
struct ReadsText { std::vector<uint8_t> bgzf; int64_t n_records = 0, raw_bytes = 0; };
void reads_encode_run(mm_ctx* ctx, const mm_seqset* reads, const ReadsSelection& sel, bool with_qual, int64_t group_bytes, ReadsText* out);
}
