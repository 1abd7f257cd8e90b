// The identity filter of an EM problem (classify --min-identity; the reference does it in util/filterLowIdentityEntities.pl; DESIGN.md section 4,
// "Identity filter"; the definition: mm_ident_core.hpp).  All of it runs on the device:
//   reads     ident_reads_kernel runs mm_ident_core.hpp's ident_read for every read, in the loop of mm_lca.hip (mm_prims.hpp, for_each_read_tile):
//             four consecutive reads per wavefront, a group of 16 lanes each with one entry per lane, for reads of <= IDENT_GROUP entries; the whole wavefront strides over a
//             longer read.  It leaves the bits of read_max[r] and of ident[best[r]] (IDENT_NONE for a read without entries: behind every
//             identity), taxon[best[r]] (n_taxa for such a read: a bucket behind every taxon) and counts the reads per taxon with 64-bit vector
//             atomics.  A maximum is the same in either shape, so the split point changes no result.
//   sort      one radix sort of the read_max bits (non-negative doubles order as their 64-bit patterns) gives sorted_max; two binary searches
//             give the number of reads with entries (the first IDENT_NONE) and n_le (the first pattern above the threshold's)
//   medians   as stage (d) of mm_gene.hip, from the same rank_by_bits: the best identities are sorted with their read indices and every read gets its global rank; the keys
//             taxon << rb | rank are radix-sorted; first[] is the scan of the reads per taxon; the median of taxon t is the identity whose rank
//             sits at first[t] + n_t / 2; removed[t] follows
//   compact   read_removed[r] from removed[]; a flag per entry (its taxon is not removed), an exclusive scan, a flag per read (its scanned range
//             is not empty), a second scan, and a scatter of the kept indices: entry_src, read_src, read_off_out
// The sorts and scans are rocprim's, through mm_prims.hpp, and share the job's one scratch buffer.  The buffers are not tiled: the job holds 12 bytes per entry on top of the inputs and 48 per read, far below the EM problem that is resident
// beside it.  Entry and read indices are 64-bit; ranks are 32-bit, hence MM_ERR_LIMIT at 2^32 reads.
#include "mm_ident.hpp"
#include "mm_prims.hpp"
#include <algorithm>
#include <limits>

namespace mm {

struct IdentOwnEntry {                                            // the one entry of this lane (0 for a lane without one: below or equal to every identity)
  uint64_t b;
  __device__ uint64_t bits(int64_t) const { return b; }
};

struct IdentReadsArgs {
  const int64_t* read_off; const int32_t* taxon; const double* ident; const int64_t* best; int64_t n_reads; int32_t n_taxa;
  uint64_t* max_bits; uint64_t* best_bits; int32_t* best_taxon; unsigned long long* taxon_reads;
};
__device__ inline void ident_store(const IdentReadsArgs& a, int64_t r, int64_t n, uint64_t mx) {
  if (n == 0) { a.max_bits[r] = IDENT_NONE; a.best_bits[r] = IDENT_NONE; a.best_taxon[r] = a.n_taxa; return; }
  const int64_t b = a.best[r];
  const int32_t t = a.taxon[b];
  a.max_bits[r] = mx; a.best_bits[r] = ident_bits(a.ident[b]); a.best_taxon[r] = t;
  atomicAdd(&a.taxon_reads[t], 1ull);
}
__global__ void __launch_bounds__(256) ident_reads_kernel(IdentReadsArgs a) {
  for_each_read_tile<IDENT_GROUP>(a.read_off, a.n_reads,
    [&](int64_t r, int64_t lo, int64_t n, bool mine, int gl) {    // the tile's short reads, and its reads without entries
      IdentOwnEntry e{0};
      if (mine && gl < n) e.b = ident_bits(a.ident[lo + gl]);
      const uint64_t mx = ident_read(Lanes<IDENT_GROUP>{}, e, mine ? n : 0);
      if (mine && gl == 0) ident_store(a, r, n, mx);
    },
    [&](int64_t r, int64_t lo, int64_t n) {                       // its long reads, one after the other
      const uint64_t mx = ident_read(Lanes<64>{}, IdentReadEntries{a.ident, lo}, n);
      if (Lanes<64>{}.lane() == 0) ident_store(a, r, n, mx);
    });
}

// first index of the ascending a[0, n) with a[i] >= x (lower) or a[i] > x (upper)
__device__ inline int64_t ident_bound(const uint64_t* a, int64_t n, uint64_t x, bool upper) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (upper ? a[mid] <= x : a[mid] < x) lo = mid + 1; else hi = mid; }
  return lo;
}
// counts[0]: reads with entries; counts[1]: n_le (le_none: the threshold is negative)
__global__ void ident_counts_kernel(const uint64_t* __restrict__ sorted, int64_t n, uint64_t thr_bits, bool le_none, int64_t* __restrict__ counts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t with = ident_bound(sorted, n, IDENT_NONE, false);
  counts[0] = with;
  counts[1] = le_none ? 0 : ident_bound(sorted, with, thr_bits, true);
}
// perm[i]: the read at global rank i of the best identities; the key of that read
__global__ void __launch_bounds__(256) ident_keys_kernel(const uint32_t* __restrict__ perm, int64_t n, const int32_t* __restrict__ best_taxon, int rb, uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[perm[i]] = (uint64_t)best_taxon[perm[i]] << rb | (uint64_t)i;
}
__global__ void __launch_bounds__(256) ident_select_kernel(int32_t n_taxa, const unsigned long long* __restrict__ taxon_reads, const int64_t* __restrict__ first,
                                                           const uint64_t* __restrict__ keys, int rb, const uint64_t* __restrict__ best_sorted, double thr,
                                                           uint64_t* __restrict__ median_bits, uint8_t* __restrict__ removed) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_taxa) return;
  const int64_t n = (int64_t)taxon_reads[t];
  uint64_t bits = IDENT_NAN_BITS;
  if (n) bits = best_sorted[keys[first[t] + ident_median_rank(n)] & ((1ull << rb) - 1)];
  median_bits[t] = bits;
  removed[t] = ident_removed(n, ident_from_bits(bits), thr) ? 1 : 0;
}
__global__ void __launch_bounds__(256) ident_read_removed_kernel(const int32_t* __restrict__ best_taxon, int64_t n, int32_t n_taxa, const uint8_t* __restrict__ removed, uint8_t* __restrict__ read_removed) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < n) read_removed[r] = best_taxon[r] < n_taxa ? removed[best_taxon[r]] : 0;
}
// keep[i] for the entries, keep[n] = 0 for the scan's total
__global__ void __launch_bounds__(256) ident_entry_flags_kernel(const int32_t* __restrict__ taxon, int64_t n, const uint8_t* __restrict__ removed, uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keep[i] = removed[taxon[i]] ? 0 : 1;
  else if (i == n) keep[i] = 0;
}
__global__ void __launch_bounds__(256) ident_read_flags_kernel(const int64_t* __restrict__ read_off, int64_t n, const int64_t* __restrict__ epos, uint8_t* __restrict__ keep) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < n) keep[r] = epos[read_off[r + 1]] > epos[read_off[r]] ? 1 : 0;
  else if (r == n) keep[r] = 0;
}
__global__ void __launch_bounds__(256) ident_scatter_entries_kernel(const uint8_t* __restrict__ keep, const int64_t* __restrict__ epos, int64_t n, int64_t* __restrict__ entry_src) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && keep[i]) entry_src[epos[i]] = i;
}
// the kept reads, and behind the last one the number of kept entries
__global__ void __launch_bounds__(256) ident_scatter_reads_kernel(const uint8_t* __restrict__ keep, const int64_t* __restrict__ rpos, int64_t n, const int64_t* __restrict__ read_off,
                                                                  const int64_t* __restrict__ epos, int64_t* __restrict__ read_src, int64_t* __restrict__ read_off_out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < n && keep[r]) { read_src[rpos[r]] = r; read_off_out[rpos[r]] = epos[read_off[r]]; }
  else if (r == n) read_off_out[rpos[n]] = epos[read_off[n]];
}

namespace {

struct IdentJob {
  const IdentIn& in; const IdentOut& out; hipStream_t st;
  StageClock<4> clk;                                               // MM_IDENT_TIMING=1: reads, sort, medians, compact on stderr
  const int64_t NR, NE; const size_t nr, ne, nt;
  DBuf<int64_t> d_off, d_best, d_counts; DBuf<int32_t> d_taxon, d_best_taxon; DBuf<double> d_ident;
  DBuf<uint64_t> d_max_bits, d_best_bits, d_sorted_max, d_best_sorted, d_median; DBuf<unsigned long long> d_taxon_reads; DBuf<uint8_t> d_removed, d_read_removed;
  DBuf<uint8_t> tmp;

  IdentJob(const IdentIn& in_, const IdentOut& out_, hipStream_t st_)
      : in(in_), out(out_), st(st_), clk(getenv("MM_IDENT_TIMING") != nullptr, st_), NR(in_.n_reads), NE(in_.read_off[in_.n_reads]), nr((size_t)NR), ne((size_t)NE), nt((size_t)in_.n_taxa) {}

  void report() const {
    if (clk.on) fprintf(stderr, "MM_IDENT_TIMING reads %.3f sort %.3f medians %.3f compact %.3f ms; %lld reads, %lld entries\n", clk.ms[0], clk.ms[1], clk.ms[2], clk.ms[3], (long long)NR, (long long)NE);
  }
  void reads() {
    d_off.alloc(nr + 1); d_off.upload(in.read_off, nr + 1, st);
    d_best.alloc(nr); d_best.upload(in.best, nr, st);
    d_taxon.alloc(ne); d_taxon.upload(in.taxon, ne, st);
    d_ident.alloc(ne); d_ident.upload(in.ident, ne, st);
    d_max_bits.alloc(nr); d_best_bits.alloc(nr); d_best_taxon.alloc(nr);
    d_taxon_reads.alloc(nt + 1); d_taxon_reads.zero(st);           // ([n_taxa] stays 0: the scan's total)
    clk.start();
    const dim3 grid(read_tile_grid<IDENT_GROUP>(NR)), blk(256);
    ident_reads_kernel<<<grid, blk, 0, st>>>(IdentReadsArgs{d_off.p, d_taxon.p, d_ident.p, d_best.p, NR, in.n_taxa, d_max_bits.p, d_best_bits.p, d_best_taxon.p, d_taxon_reads.p});
    MM_KERNEL_CHECK();
    clk.stop(0);
  }
  void sort_max() {
    clk.start();
    d_sorted_max.alloc(nr); d_counts.alloc(2);
    sort_keys(tmp, d_max_bits.p, d_sorted_max.p, nr, 0, 64, st);
    ident_counts_kernel<<<dim3(1), dim3(64), 0, st>>>(d_sorted_max.p, NR, ident_bits(in.thr < 0 ? 0.0 : in.thr), in.thr < 0, d_counts.p); MM_KERNEL_CHECK();
    const std::vector<int64_t> c = d_counts.to_host(st);
    clk.stop(1);
    *out.n_with_entries = c[0]; *out.n_le = c[1];
    static_assert(sizeof(double) == sizeof(uint64_t), "identities are copied as bit patterns");
    d_sorted_max.download((uint64_t*)out.sorted_max, (size_t)c[0], st);
  }
  void medians() {
    clk.start();
    const int rb = bits_for((uint64_t)NR), tb = bits_for((uint64_t)in.n_taxa);
    DBuf<uint32_t> d_iota(nr), d_perm(nr); DBuf<uint64_t> d_keys(nr), d_keys2(nr); DBuf<int64_t> d_first(nt + 1);
    d_best_sorted.alloc(nr); d_median.alloc(std::max<size_t>(nt, 1)); d_removed.alloc(std::max<size_t>(nt, 1));
    rank_by_bits(tmp, d_best_bits.p, d_best_sorted.p, d_iota.p, d_perm.p, nr, st);
    ident_keys_kernel<<<dim3(flat_grid(NR)), dim3(256), 0, st>>>(d_perm.p, NR, d_best_taxon.p, rb, d_keys.p); MM_KERNEL_CHECK();
    sort_keys(tmp, d_keys.p, d_keys2.p, nr, 0, rb + tb, st);
    exclusive_scan(tmp, d_taxon_reads.p, d_first.p, nt + 1, st);
    ident_select_kernel<<<dim3(flat_grid(in.n_taxa)), dim3(256), 0, st>>>(in.n_taxa, d_taxon_reads.p, d_first.p, d_keys2.p, rb, d_best_sorted.p, in.thr, d_median.p, d_removed.p);
    MM_KERNEL_CHECK();
    d_read_removed.alloc(nr);
    ident_read_removed_kernel<<<dim3(flat_grid(NR)), dim3(256), 0, st>>>(d_best_taxon.p, NR, in.n_taxa, d_removed.p, d_read_removed.p); MM_KERNEL_CHECK();
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are copied as they lie");
    d_taxon_reads.download((unsigned long long*)out.taxon_reads, nt, st);
    d_median.download((uint64_t*)out.taxon_median, nt, st);
    d_removed.download(out.taxon_removed, nt, st);
    d_read_removed.download(out.read_removed, nr, st);
    MM_HIP(mm::stream_sync(st));                                   // (the buffers of this scope)
    clk.stop(2);
  }
  void compact() {
    clk.start();
    DBuf<uint8_t> d_ekeep(ne + 1), d_rkeep(nr + 1); DBuf<int64_t> d_epos(ne + 1), d_rpos(nr + 1), d_entry_src(ne), d_read_src(nr), d_off_out(nr + 1);
    ident_entry_flags_kernel<<<dim3(flat_grid(NE + 1)), dim3(256), 0, st>>>(d_taxon.p, NE, d_removed.p, d_ekeep.p); MM_KERNEL_CHECK();
    exclusive_scan(tmp, d_ekeep.p, d_epos.p, ne + 1, st);
    ident_read_flags_kernel<<<dim3(flat_grid(NR + 1)), dim3(256), 0, st>>>(d_off.p, NR, d_epos.p, d_rkeep.p); MM_KERNEL_CHECK();
    exclusive_scan(tmp, d_rkeep.p, d_rpos.p, nr + 1, st);
    ident_scatter_entries_kernel<<<dim3(flat_grid(NE)), dim3(256), 0, st>>>(d_ekeep.p, d_epos.p, NE, d_entry_src.p); MM_KERNEL_CHECK();
    ident_scatter_reads_kernel<<<dim3(flat_grid(NR + 1)), dim3(256), 0, st>>>(d_rkeep.p, d_rpos.p, NR, d_off.p, d_epos.p, d_read_src.p, d_off_out.p); MM_KERNEL_CHECK();
    int64_t n_e = 0, n_r = 0;
    d_epos.download(&n_e, 1, st, ne); d_rpos.download(&n_r, 1, st, nr);
    MM_HIP(mm::stream_sync(st));
    d_entry_src.download(out.entry_src, (size_t)n_e, st); d_read_src.download(out.read_src, (size_t)n_r, st); d_off_out.download(out.read_off_out, (size_t)n_r + 1, st);
    MM_HIP(mm::stream_sync(st));
    clk.stop(3);
    *out.n_entries_out = n_e; *out.n_reads_out = n_r;
  }
};

}  // namespace

void ident_filter_run(mm_ctx* ctx, const IdentIn& in, const IdentOut& out) {
  const int bad = ident_args_check(in.n_reads, in.read_off, in.taxon, in.ident, in.best, in.n_taxa, in.thr);
  MM_REQUIRE(!bad, MM_ERR_ARG, std::string("mm_ident_filter: ") + ident_arg_message(bad));
  MM_REQUIRE(in.n_reads < ((int64_t)1 << 32), MM_ERR_LIMIT, "mm_ident_filter: 2^32 reads or more in one call");
  const bool filtered = out.read_src != nullptr;
  std::fill(out.taxon_reads, out.taxon_reads + in.n_taxa, (int64_t)0);
  std::fill(out.taxon_median, out.taxon_median + in.n_taxa, std::numeric_limits<double>::quiet_NaN());
  std::fill(out.taxon_removed, out.taxon_removed + in.n_taxa, (uint8_t)0);
  std::fill(out.read_removed, out.read_removed + in.n_reads, (uint8_t)0);
  *out.n_with_entries = 0; *out.n_le = 0;
  if (filtered) { *out.n_reads_out = 0; *out.n_entries_out = 0; out.read_off_out[0] = 0; }
  if (in.read_off[in.n_reads] == 0) return;                        // no entry: nothing to sort, nothing removed, nothing kept
  IdentJob J(in, out, ctx->stream);
  J.reads();
  J.sort_max();
  J.medians();
  if (filtered) J.compact();
  MM_HIP(mm::stream_sync(J.st));
  J.report();
}

}  // namespace mm
