// Host-side entries of the device codecs: BGZF inflate (mm_inflate.hip), BGZF deflate (mm_deflate.hip), plain gzip (mm_gzip.hip).
// Declarations only: the codecs' own headers (mm_inflate.hpp, mm_deflate.hpp, mm_gzip.hpp) hold their device code, which callers need not compile.
#pragma once
#include "mm_common.hpp"

namespace mm {
int64_t bgzf_inflate(mm_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, const int64_t* comp_off, const int32_t* comp_len, int32_t n,
                     uint8_t* out, int64_t out_cap, const int64_t* out_off, int32_t* status);
// BGZF blocks of the host's inflated into a buffer of the device's, where they stay
int64_t bgzf_inflate_resident(mm_ctx* ctx, const uint8_t* const* block, const int32_t* comp_len, int32_t n, uint8_t* d_out, int64_t out_cap, const int64_t* out_off,
                              int32_t* status);
void bgzf_deflate(mm_ctx* ctx, const uint8_t* in, int64_t in_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes, int32_t* n_blocks);
int64_t bgzf_deflate_bound(int64_t in_bytes);
// BGZF members of input that lies on the device
void bgzf_deflate_resident(mm_ctx* ctx, const uint8_t* d_in, int64_t in_bytes, int64_t n, uint8_t* down, int32_t* sizes);
mm_gzip* gzip_open(mm_ctx* ctx, int64_t chunk, int64_t segment);
void gzip_close(mm_gzip* g);
int gzip_feed(mm_gzip* g, const uint8_t* comp, int64_t n, bool last, int64_t* avail);
int64_t gzip_read(mm_gzip* g, uint8_t* out, int64_t cap);
void gzip_stats(const mm_gzip* g, int64_t* counts, double* seconds);
mm_ctx* gzip_ctx(const mm_gzip* g);
}
