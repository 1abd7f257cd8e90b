// What the per-job kernels of mm_pileup.hip and mm_vcf.hip share (included by those two files only): the device's lane policy, a job's arrays on the
// device, and the reduction and the interval sort that mm_pileup.hip defines.
#pragma once
#include "mm_common.hpp"
#include "mm_edit_seq.hpp"
#include <string>
#include <vector>

namespace mm {

struct PileWaveLanes {                                            // one lane per thread of a 64-thread workgroup
  static constexpr uint32_t W = 64;
  __device__ uint32_t lane() const { return threadIdx.x; }
  __device__ int64_t scan_add(int64_t v, int64_t* total) const {
    long long x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long y = __shfl_up(x, o, 64); if ((int)threadIdx.x >= o) x += y; }
    *total = (int64_t)__shfl(x, 63, 64);
    return (int64_t)x - v;
  }
  __device__ uint64_t ballot(bool b) const { return (uint64_t)__ballot(b); }
  __device__ int64_t pick(int64_t v, uint32_t l) const { return (int64_t)__shfl((long long)v, (int)l, 64); }
};
struct PileBytes { EditSeq s; int64_t g0; __device__ uint8_t byte(int64_t i) const { return s.byte(g0 + i); } };   // read (or contig) coordinate -> the set's byte

struct PileJobs {
  int64_t n; const int32_t* read; const int32_t* strand; const int32_t* contig; const int32_t* dist; const int64_t* first;
  const int64_t* op_off; const uint32_t* ops; const uint8_t* use;
};
constexpr unsigned long long PILE_NO_ERROR = ~0ull;
constexpr int64_t PILE_GRID_MAX = (int64_t)1 << 30;               // workgroups per launch

// op_off starts at 0 or more and never falls (MM_ERR_ARG in the name of `who`)
void pile_offsets_check(const int64_t* off, int64_t n, const char* who);
// The segments of equal keys of sorted[0, n), n > 0, into host memory: their keys, and their counts — the segments' lengths, or with d_counts (in the order
// of sorted, n + 1 entries, the last one 0) the sums of their counts.  With `second` a key is the pair (sorted[i], second[i]) and keys2 gets the second
// words.  Returns false where a sum passes 2^32 - 1.
bool reduce_sorted(DBuf<uint8_t>& tmp, const uint64_t* sorted, const uint64_t* second, const uint32_t* d_counts, int64_t n, hipStream_t st, std::vector<uint64_t>* keys,
                   std::vector<uint64_t>* keys2, std::vector<uint32_t>* counts);
// The interval keys (mmp::interval_key) of n > 0 alignments given in host arrays: starts ascending with end_of[i] the end that belongs to starts[i], ends
// ascending; each buffer holds n words.  bits: 32 + contig_bits of the reference.
void sorted_interval_keys(DBuf<uint8_t>& tmp, int64_t n, const int32_t* contig, const int64_t* first, const int64_t* last, int bits, hipStream_t st, DBuf<uint64_t>& starts,
                          DBuf<uint64_t>& end_of, DBuf<uint64_t>& ends);
int contig_bits(int64_t n_contigs);                               // the bits that hold every contig index

}  // namespace mm
