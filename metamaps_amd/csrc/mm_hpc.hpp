// Homopolymer compression of an uploaded sequence set on the device, and the map from compressed to raw coordinates (mm_hpc.hip).
#pragma once
#include "mm_common.hpp"
#include "mm_hpc_core.hpp"

// Compressed -> raw coordinates of one compressed set: the run-start bitmap over the raw packed stream (1 bit per raw stream position) and
// the raw position of every 512th kept base of each sequence: 0.125 + 4 / 512 bytes per raw base at most (the packed raw set is 0.25).
struct mm_hpc_map {
  mm_ctx* ctx = nullptr;
  int64_t n = 0;
  std::vector<int32_t> rawlen, clen;
  mm::DBuf<uint64_t> bitmap, d_base, d_samp_off;
  mm::DBuf<int32_t> d_rawlen, d_clen;
  mm::DBuf<uint32_t> samp;
  mm::HpcMapView view() const { return mm::HpcMapView{bitmap.p, d_base.p, d_rawlen.p, d_clen.p, d_samp_off.p, samp.p, n}; }
  size_t device_bytes() const { return bitmap.bytes() + d_base.bytes() + d_samp_off.bytes() + d_rawlen.bytes() + d_clen.bytes() + samp.bytes(); }
};
struct mm_mapping;

namespace mm {
// out = hpc(raw), in the layout of an uploaded set; map (may be null) receives the coordinate map
void seqset_hpc(mm_ctx* ctx, const mm_seqset* raw, mm_seqset* out, mm_hpc_map* map);
void hpc_map_to_raw(mm_hpc_map* map, const int32_t* seq, const int64_t* pos, int64_t n, int64_t* first_out, int64_t* last_out);
// the records' ref_start -> raw(contig, start); end_out[i] = rawlast(contig, start + compressed read length - 1)
void mapping_to_raw(mm_ctx* ctx, mm_mapping* m, const mm_hpc_map* ref_map, int64_t* end_out, int64_t cap);
}
