// BAM records of a batch of aligned jobs, encoded and deflated on the device (mm_bam.hip; the record: mm_bam_core.hpp).
#pragma once
#include "mm_jobs_dev.hpp"
#include "mm_codec.hpp"                                            // (bgzf_deflate_resident: BGZF members of input that lies on the device)
#include <vector>

namespace mm {
// the columns that the BAM record alone reads, beside the aligned jobs (mm_jobs_dev.hpp): the caller's arrays as mm_bam_encode takes them, or their copies on the device
struct BamColumns { const uint16_t* flag; const uint8_t* mapq; const int64_t* name_off; const char* names; };
// the members of every group back to back, in host memory; the records in the order of the inflated stream: record i is job rec_job[i]'s and lies at
// [rec_off[i], rec_off[i + 1])
struct BamMembers { std::vector<uint8_t> bgzf; std::vector<int64_t> rec_job, rec_off = std::vector<int64_t>(1, 0); int64_t n_records = 0, raw_bytes = 0; };
constexpr int64_t BAM_GROUP_BYTES = (int64_t)4096 * 0xff00;       // group_bytes 0: what one launch of the deflate kernel takes (255 MiB of records)
void bam_encode_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const AlignedJobsIn& jobs, const BamColumns& in, int64_t group_bytes, bool sorted, BamMembers* out);   // sorted: the records ascending by (contig, first, job)
}
