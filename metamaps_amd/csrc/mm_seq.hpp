// Sequence sets (mm_seq.hip): packing and upload, files, slices and concatenations, fetch.  The struct itself is mm_common.hpp's mm_seqset.
#pragma once
#include "mm_common.hpp"

namespace mm {
void seqset_upload(mm_seqset* s);
void seqset_upload_nt16(mm_seqset* s);
void seqset_upload_qual(mm_seqset* s);                           // the quality plane of the staged sequences, called by the two above
void seqset_fetch_qual(mm_seqset* s, int64_t i, uint8_t* out, int64_t cap);
void seqset_save(mm_seqset* s, const char* path);
void seqset_load(mm_seqset* s, const char* path);
void seqset_fetch(mm_seqset* s, int64_t i, char* out, int64_t cap);
void seqset_fetch_range(mm_seqset* s, int64_t first, int64_t count, char* out, int64_t cap);
void seqset_slice(const mm_seqset* s, int64_t first, int64_t count, mm_seqset* o);
void seqset_concat(const mm_seqset* const* parts, int n_parts, mm_seqset* o);
}
