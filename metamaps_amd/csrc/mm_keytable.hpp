// A table of (key, count) rows whose key is one or two 64-bit words: the pileup's and the modifications' (key, count) pairs and the VCF's (w0, w1, count)
// triples, sorted, reduced, merged and finished by one pipeline (mm_keytable.hip; DESIGN.md section 1, "Key tables"; the events that fill a table:
// mm_events.hpp).  The pipeline reads no field of a key but, in the finish, the contig and the position that the pileup's and the VCF's formats hold in w0
// (mm_pileup_core.hpp: key_contig, key_pos); what a key means stays with mm_pileup.hip, mm_vcf.hip and mm_mods.hip.
#pragma once
#include "mm_common.hpp"
#include "mm_edit_seq.hpp"
#include "mm_pileup_core.hpp"
#include "mm_prims.hpp"
#include <functional>
#include <vector>

namespace mm {

// rows with unique keys in ascending order of (w0, w1), in host memory; w1 is empty for a table of one-word keys
struct KeyTable {
  std::vector<uint64_t> w0, w1; std::vector<uint32_t> counts;
  void clear() { w0.clear(); w1.clear(); counts.clear(); }
};

// A table sorted on the device: w0 ascending, with w1 the second words behind them, with counts the counts behind them and a last entry 0 (the scan's total).
struct SortedTable { DBuf<uint64_t> w0, w1; DBuf<uint32_t> counts, perm, i1; };   // (perm, i1: the two-word order's indexes, which no launch may outlive)
// The rows (w0[i], w1[i], counts[i]), i < n < 2^32, in key order by the bits [0, bits0) of w0 and [0, bits1) of w1; w1 and counts may be null.  One-word
// keys take one radix sort of the keys (with the counts as its values); two-word keys two stable passes over an index: by w1, then by w0.
void sort_table(DBuf<uint8_t>& tmp, uint64_t* w0, uint64_t* w1, uint32_t* counts, int64_t n, int bits0, int bits1, hipStream_t st, SortedTable* s);
// The segments of equal keys of a sorted table of n > 0 rows into host memory: their keys, and their counts — the segments' lengths, or with s.counts the sums
// of their counts.  Returns false where a sum passes 2^32 - 1.
bool reduce_sorted(DBuf<uint8_t>& tmp, const SortedTable& s, int64_t n, hipStream_t st, KeyTable* out);
// mm_pileup_merge, mm_mod_merge and mm_vcf_merge (w1 null: one-word keys): the rows summed by key.  who: the entry point's name; timing_env: the variable that asks for
// the stage times, and the word its line starts with.
void merge_run(mm_ctx* ctx, int64_t n, const uint64_t* w0, const uint64_t* w1, const uint32_t* counts, const char* who, const char* timing_env, KeyTable* out);

int contig_bits(int64_t n_contigs);                               // the bits that hold every contig index
// The interval keys (mmp::interval_key) of n > 0 alignments given in host arrays: starts ascending with end_of[i] the end that belongs to starts[i], ends
// ascending; each buffer holds n words.  bits: 32 + contig_bits of the reference.
struct SortedIntervals { DBuf<uint64_t> starts, end_of, ends; };
struct FinishIn;
// in.n_iv > 0 intervals, already checked against their contigs, uploaded and sorted into iv, whose buffers the caller has allocated (mm_depth.hip shares it)
void sorted_interval_keys(DBuf<uint8_t>& tmp, const FinishIn& in, int bits, hipStream_t st, SortedIntervals& iv);

// a merged table, the intervals of the contributing alignments and the two thresholds, as mm_pileup_finish and mm_vcf_finish take them (w1 null: one-word keys)
struct FinishIn {
  int64_t n; const uint64_t* w0; const uint64_t* w1; const uint32_t* counts;
  int64_t n_iv; const int32_t* iv_contig; const int64_t* iv_first; const int64_t* iv_last;
  int64_t min_count; double min_frac;
};
struct KeptRows { std::vector<uint64_t> w0; std::vector<uint32_t> count, depth; };   // the kept rows in key order: what every format's result starts with
// what a compaction reads and writes: row i with keep[i] goes to place pos[i]
struct KeptDev {
  int64_t n; const uint64_t* w0; const uint32_t* counts; const uint32_t* depth; const uint8_t* keep; const int64_t* pos;
  uint64_t* o0; uint32_t* ocount; uint32_t* odepth;
};
// pay(i, o, contig, position): what the format adds to the kept row i at its place o (its buffers are its own)
template <class Payload> __global__ void __launch_bounds__(256) kept_compact_kernel(KeptDev v, Payload pay) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= v.n || !v.keep[i]) return;
  const int64_t o = v.pos[i];
  v.o0[o] = v.w0[i]; v.ocount[o] = v.counts[i]; v.odepth[o] = v.depth[i];
  pay(i, o, mmp::key_contig(v.w0[i]), mmp::key_pos(v.w0[i]));
}
template <class Payload> void compact_kept(const KeptDev& v, const Payload& pay, hipStream_t st) {
  kept_compact_kernel<<<dim3(flat_grid(v.n)), dim3(256), 0, st>>>(v, pay); MM_KERNEL_CHECK();
}
// What the two finishes share.  The requires on the reference and the thresholds, check_keys() (the format's own: what a valid key is), the interval checks;
// then, unless there is no row and no interval that `iv` would keep (returns false, nothing launched): the intervals uploaded and sorted (clk.ms[0]); the rows
// uploaded, a row's depth from two binary searches, its keep flag, a scan, compact(rows) (the format's compact_kept) and the kept rows fetched: stage 1 of
// clk, started here and stopped by the format once it has fetched what its payload wrote.  iv: null where the format has no use for the sorted intervals afterwards.
bool finish_kept(mm_ctx* ctx, const mm_seqset* ref, const FinishIn& in, const char* who, const std::function<void()>& check_keys, const std::function<void(const KeptDev&)>& compact,
                 StageClock<3>& clk, SortedIntervals* iv, KeptRows* out);

}  // namespace mm
