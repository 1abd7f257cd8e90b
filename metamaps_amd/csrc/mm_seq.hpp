// Sequence sets (mm_seq.hip): packing and upload, files, slices and concatenations, fetch.  The struct itself is mm_common.hpp's mm_seqset.
#pragma once
#include "mm_common.hpp"

namespace mm {
void seqset_upload(mm_seqset* s);
void seqset_upload_nt16(mm_seqset* s);
void seqset_upload_qual(mm_seqset* s);                           // the quality plane of the staged sequences, called by the two above
void seqset_fetch_qual(mm_seqset* s, int64_t i, uint8_t* out, int64_t cap);
// mm_seqset_add_mods: the groups of the sequence added last into the set's staging, after the argument checks; the (who, prob) plane of the staged
// groups, called by the two uploads behind the bases; a sequence's stored calls (mm_mods.hip)
void seqset_add_mods(mm_seqset* s, int32_t n_groups, const uint8_t* base, const int8_t* code, const uint8_t* mode, const int64_t* off, const uint32_t* skips, const uint8_t* ml);
void seqset_upload_mods(mm_seqset* s);
void seqset_fetch_mods(mm_seqset* s, int64_t i, uint8_t* who, uint8_t* prob, int64_t cap);
void seqset_save(mm_seqset* s, const char* path);
void seqset_load(mm_seqset* s, const char* path);
void seqset_fetch(mm_seqset* s, int64_t i, char* out, int64_t cap);
void seqset_fetch_range(mm_seqset* s, int64_t first, int64_t count, char* out, int64_t cap);
void seqset_slice(const mm_seqset* s, int64_t first, int64_t count, mm_seqset* o);
void seqset_concat(const mm_seqset* const* parts, int n_parts, mm_seqset* o);
}
