// The identity filter of classify --min-identity (the reference's util/filterLowIdentityEntities.pl; DESIGN.md section 4, "Identity filter"): which
// genomes of an EM problem are removed because the median identity of their best mappings lies below a threshold, and the EM problem that is left.
//   input        reads r with entries [read_off[r], read_off[r+1]); taxon[i]; best[r], an entry of read r (what reads2Taxon uses); ident[i], the
//                entry's identity in PERCENT (0-based field 12 of the mapping line)
//   read_max[r]  the largest ident of the read's entries; sorted_max: the read_max of the reads with entries, ascending; n_le: how many are <= thr
//   taxon t      I(t) = the ident[best[r]] of the reads with taxon[best[r]] == t; taxon_reads[t] = |I(t)|; taxon_median[t] = the element of 0-based
//                rank |I(t)| / 2 of I(t) in ascending order (the UPPER median, the script's int(n / 2)), NaN where I(t) is empty
//   removed[t]   taxon_reads[t] > 0 && taxon_median[t] < thr (strictly, in double; thr in percent)
//   read         read_removed[r] = removed[taxon[best[r]]]; a read without entries is neither removed nor kept
//   filtered     an entry is kept iff its taxon is not removed, a read iff it keeps an entry: entry_src / read_src (original indices, ascending),
//                read_off_out (offsets of the kept reads into entry_src)
// Identities are non-negative (a -0.0 is taken as 0), so they order as their 64-bit patterns do: what the device sorts (ident_bits).
// The pass over a read (ident_read) is one text for a serial caller, a group of 16 lanes with an entry each, and a wavefront striding over a long
// read: the lanes G give lane(), width() and max().  ident_filter_host is the whole definition on one host thread.
//
// Compiles for host (tests/test_ident_core.cpp via g++, tools/ident_host_filter.cpp) and device (mm_ident.hip).
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef MM_HD
#if defined(__HIPCC__)
#define MM_HD __host__ __device__ inline
#else
#define MM_HD inline
#endif
#endif

namespace mm {

constexpr uint64_t IDENT_NONE = ~(uint64_t)0;                     // in place of an identity's bits: a read without entries (sorts behind every identity)
constexpr uint64_t IDENT_NAN_BITS = 0x7ff8000000000000ull;

MM_HD uint64_t ident_bits(double x) { x += 0.0; uint64_t b; memcpy(&b, &x, 8); return b; }   // (-0.0 + 0.0 is +0.0)
MM_HD double ident_from_bits(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }
MM_HD int64_t ident_median_rank(int64_t n) { return n / 2; }
MM_HD bool ident_removed(int64_t n, double median, double thr) { return n > 0 && median < thr; }

struct IdentSerial {                                              // one lane on its own
  MM_HD int lane() const { return 0; }
  MM_HD int width() const { return 1; }
  MM_HD uint64_t max(uint64_t x) const { return x; }
};
struct IdentReadEntries {                                         // entry k of the read whose entries begin at lo
  const double* ident; int64_t lo;
  MM_HD uint64_t bits(int64_t k) const { return ident_bits(ident[lo + k]); }
};
// the bits of read_max of a read of n > 0 entries; every lane of g returns it
template <class G, class E> MM_HD uint64_t ident_read(const G& g, const E& e, int64_t n) {
  uint64_t m = 0;
  for (int64_t k = g.lane(); k < n; k += g.width()) { const uint64_t b = e.bits(k); m = b > m ? b : m; }
  return g.max(m);
}

// ---- the arguments of mm_ident_filter (host): 0 if fine, else which rule is broken (ident_arg_message)
enum IdentArgError { IDENT_OK = 0, IDENT_BAD_SIZE, IDENT_BAD_OFFSETS, IDENT_BAD_TAXON, IDENT_BAD_BEST, IDENT_BAD_IDENTITY, IDENT_BAD_THRESHOLD };
inline const char* ident_arg_message(int e) {
  static const char* const M[] = {"", "a negative size", "read_off must start at 0 and ascend", "a taxon lies outside [0, n_taxa)",
                                  "a best[r] lies outside its read's entries", "an identity is negative or not a number", "the threshold is not a number"};
  return e >= 0 && e < (int)(sizeof M / sizeof M[0]) ? M[e] : "?";
}
inline int ident_args_check(int64_t n_reads, const int64_t* read_off, const int32_t* taxon, const double* ident, const int64_t* best, int64_t n_taxa, double thr) {
  if (n_reads < 0 || n_taxa < 0) return IDENT_BAD_SIZE;
  if (!read_off || read_off[0] != 0) return IDENT_BAD_OFFSETS;
  for (int64_t r = 0; r < n_reads; ++r) if (read_off[r + 1] < read_off[r]) return IDENT_BAD_OFFSETS;
  for (int64_t i = 0; i < read_off[n_reads]; ++i) {
    if (taxon[i] < 0 || taxon[i] >= n_taxa) return IDENT_BAD_TAXON;
    if (!(ident[i] >= 0)) return IDENT_BAD_IDENTITY;               // (a NaN is refused)
  }
  for (int64_t r = 0; r < n_reads; ++r)
    if (read_off[r + 1] > read_off[r] && (best[r] < read_off[r] || best[r] >= read_off[r + 1])) return IDENT_BAD_BEST;
  if (thr != thr) return IDENT_BAD_THRESHOLD;
  return IDENT_OK;
}

}  // namespace mm

// ---- the whole definition on one host thread (the tests' and tools' host build; the library runs mm_ident.hip) ----
#include <algorithm>
#include <vector>

namespace mm {

struct IdentHostOut {
  std::vector<double> sorted_max, taxon_median; int64_t n_le = 0;
  std::vector<int64_t> taxon_reads, read_src, entry_src, read_off_out;
  std::vector<uint8_t> taxon_removed, read_removed;
};
// (arguments as ident_args_check accepts them)
inline void ident_filter_host(int64_t n_reads, const int64_t* read_off, const int32_t* taxon, const double* ident, const int64_t* best, int64_t n_taxa, double thr,
                              IdentHostOut* o) {
  std::vector<uint64_t> mx;
  std::vector<std::vector<uint64_t>> per((size_t)n_taxa);
  for (int64_t r = 0; r < n_reads; ++r) {
    const int64_t lo = read_off[r], n = read_off[r + 1] - lo;
    if (n == 0) continue;
    mx.push_back(ident_read(IdentSerial{}, IdentReadEntries{ident, lo}, n));
    per[(size_t)taxon[best[r]]].push_back(ident_bits(ident[best[r]]));
  }
  std::sort(mx.begin(), mx.end());
  o->sorted_max.clear(); o->n_le = 0;
  for (uint64_t b : mx) { o->sorted_max.push_back(ident_from_bits(b)); o->n_le += ident_from_bits(b) <= thr; }
  o->taxon_reads.assign((size_t)n_taxa, 0); o->taxon_median.assign((size_t)n_taxa, ident_from_bits(IDENT_NAN_BITS)); o->taxon_removed.assign((size_t)n_taxa, 0);
  for (size_t t = 0; t < (size_t)n_taxa; ++t) {
    std::vector<uint64_t>& x = per[t];
    o->taxon_reads[t] = (int64_t)x.size();
    if (x.empty()) continue;
    std::nth_element(x.begin(), x.begin() + ident_median_rank((int64_t)x.size()), x.end());
    o->taxon_median[t] = ident_from_bits(x[(size_t)ident_median_rank((int64_t)x.size())]);
    o->taxon_removed[t] = ident_removed((int64_t)x.size(), o->taxon_median[t], thr);
  }
  o->read_removed.assign((size_t)n_reads, 0); o->read_src.clear(); o->entry_src.clear(); o->read_off_out.assign(1, 0);
  for (int64_t r = 0; r < n_reads; ++r) {
    if (read_off[r + 1] > read_off[r]) o->read_removed[(size_t)r] = o->taxon_removed[(size_t)taxon[best[r]]];
    const size_t before = o->entry_src.size();
    for (int64_t i = read_off[r]; i < read_off[r + 1]; ++i) if (!o->taxon_removed[(size_t)taxon[i]]) o->entry_src.push_back(i);
    if (o->entry_src.size() > before) { o->read_src.push_back(r); o->read_off_out.push_back((int64_t)o->entry_src.size()); }
  }
}

}  // namespace mm
