// Exact edit distances of mappings on the device (mm_edit.hip; the definition: mm_edit_core.hpp; the recurrence and its schedule: mm_edit_bv_core.hpp)
// and their base-level alignments (the storing pass and the walk: mm_edit_trace_core.hpp).
#pragma once
#include "mm_common.hpp"
#include "mm_map.hpp"
#include "mm_edit_bv_core.hpp"
#include <vector>

namespace mm {
// arbitrary jobs, checked on the host (edit_job_check) before anything is launched; dist -1, begin = end = -1: not aligned
struct EditInfixIn { int64_t n_jobs; const int32_t* read; const int32_t* strand; const int32_t* contig; const int64_t* ws; const int64_t* we; const int32_t* max_dist; };
void edit_infix_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const EditInfixIn& in, int32_t* dist, int64_t* begin, int64_t* end);
// one job per record of the mapping by the window and cap rules; first / last: 0-based inclusive contig coordinates, -1 -1 -1: not aligned
void edit_mapping_run(mm_ctx* ctx, const mm_mapping* M, const mm_seqset* reads, const mm_seqset* reference, float pi, int32_t* dist, int64_t* first, int64_t* last, int64_t cap);
// the same jobs with their alignments: dist / first / last as the two above give them; the runs of job i are ops[op_off[i], op_off[i + 1]) (BAM's words)
struct EditAlignment { std::vector<int32_t> dist; std::vector<int64_t> first, last, op_off; std::vector<uint32_t> ops; };
void edit_infix_align_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const EditInfixIn& in, EditAlignment* out);
void edit_mapping_align_run(mm_ctx* ctx, const mm_mapping* M, const mm_seqset* reads, const mm_seqset* reference, float pi, EditAlignment* out);
}
