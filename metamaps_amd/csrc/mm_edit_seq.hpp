// The bases of a packed sequence set as the per-job kernels read them (mm_edit.hip: the alignment's symbols; mm_bam.hip: the bytes of SEQ and MD).
// An exception run holds a byte other than A C G T (mm_seq.hip upper-cases before it packs); every other base is its 2-bit code.
#pragma once
#include "mm_common.hpp"
#include "mm_edit_bv_core.hpp"
#include "mm_prims.hpp"

namespace mm {

struct EditSeq {                                                  // the bases of a set by stream coordinate; the runs may be narrowed to a stretch
  const uint32_t* packed; const uint64_t* exc_start; const uint32_t* exc_len; const uint8_t* exc_byte; int64_t n_exc; int rounds;
  // first run that ends behind g, in `rounds` rounds (2^rounds > n_exc)
  __device__ int64_t lower(uint64_t g) const {
    int64_t lo = 0, hi = n_exc;
    for (int r = 0; r < rounds; ++r)
      if (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (exc_start[mid] + exc_len[mid] <= g) lo = mid + 1; else hi = mid; }
    return lo;
  }
  __device__ uint32_t sym(int64_t g) const {
    if (n_exc) { const int64_t r = lower((uint64_t)g); if (r < n_exc && exc_start[r] <= (uint64_t)g) return BV_SYM_NONE; }
    return (packed[g >> 4] >> (2 * (g & 15))) & 3u;
  }
  __device__ uint8_t byte(int64_t g) const {                      // the byte the set holds there: the run's, or the code's letter
    if (n_exc) { const int64_t r = lower((uint64_t)g); if (r < n_exc && exc_start[r] <= (uint64_t)g) return exc_byte[r]; }
    return ascii_of_code((packed[g >> 4] >> (2 * (g & 15))) & 3u);
  }
  // the bytes of g .. g + 3, all four inside one sequence, as one little-endian word: eight bits cut out of one or two packed words, or byte by byte
  // where a run touches them
  __device__ uint32_t bytes4(int64_t g) const {
    if (n_exc) {
      const int64_t r = lower((uint64_t)g);
      if (r < n_exc && exc_start[r] < (uint64_t)g + 4) return (uint32_t)byte(g) | (uint32_t)byte(g + 1) << 8 | (uint32_t)byte(g + 2) << 16 | (uint32_t)byte(g + 3) << 24;
    }
    const uint32_t sh = 2 * (uint32_t)(g & 15);
    uint32_t c = packed[g >> 4] >> sh;
    if (sh > 24) c |= packed[(g >> 4) + 1] << (32 - sh);
    return (uint32_t)ascii_of_code(c & 3u) | (uint32_t)ascii_of_code((c >> 2) & 3u) << 8 | (uint32_t)ascii_of_code((c >> 4) & 3u) << 16 | (uint32_t)ascii_of_code((c >> 6) & 3u) << 24;
  }
  __device__ EditSeq narrowed(uint64_t g0, uint64_t g1) const {   // the runs that touch [g0, g1)
    EditSeq s = *this;
    if (!n_exc) return s;
    const int64_t r0 = lower(g0), r1 = g1 > g0 ? lower(g1 - 1) : r0;
    const int64_t end = r1 < n_exc && exc_start[r1] < g1 ? r1 + 1 : r1;
    s.exc_start += r0; s.exc_len += r0; s.exc_byte += r0; s.n_exc = end > r0 ? end - r0 : 0;
    return s;
  }
};
static EditSeq edit_seq(const mm_seqset* S) { return EditSeq{S->packed.p, S->exc_start.p, S->exc_len.p, S->exc_byte.p, S->n_exc, bits_for((uint64_t)S->n_exc)}; }

}  // namespace mm
