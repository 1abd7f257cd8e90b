// The key tables of the pileup, of the VCF and of the base modifications on the device (mm_keytable.hpp; DESIGN.md section 1, "Key tables"; the stages that
// lead from a batch's jobs to sort and reduce: mm_events.hpp).
//   sort     one-word keys: one radix sort of the keys over the bits in use (sort_pairs where counts ride along).  Two-word keys: two stable radix passes
//            over an index, by w1 and then by w0, and the words (and counts) gathered behind the index.
//   reduce   head flags, a scan and a scatter of (key, first index): mm_ident.hip's compaction.  A segment's count is its length, or the difference of one
//            64-bit prefix sum of the counts.
//   finish   the intervals' start keys (with their ends) and end keys sorted; a row's depth from two binary searches; kept rows compacted with the format's
//            payload (kept_compact_kernel).
// No kernel here waits for another workgroup; the only atomic is the minimum that marks a sum beyond 32 bits.
#include "mm_keytable.hpp"
#include <string>

namespace mm {

// dst[i] = src[idx[i]] for i < n; dst[n .. n_dst) = 0 (the counts' last entry: the scan's total)
template <class T> __global__ void __launch_bounds__(256) table_gather_kernel(const T* __restrict__ src, const uint32_t* __restrict__ idx, int64_t n, int64_t n_dst, T* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
  else if (i < n_dst) dst[i] = 0;
}
// head[i]: row i starts a segment of equal keys; head[n] = 0 for the scan's total.  A key is sorted[i], with `second` the pair (sorted[i], second[i]).
__global__ void __launch_bounds__(256) table_heads_kernel(const uint64_t* __restrict__ sorted, const uint64_t* __restrict__ second, int64_t n, uint8_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) head[i] = i == 0 || sorted[i] != sorted[i - 1] || (second && second[i] != second[i - 1]) ? 1 : 0;
  else if (i == n) head[i] = 0;
}
// the segments' keys and first indexes; start[number of segments] = n
__global__ void __launch_bounds__(256) table_segments_kernel(const uint64_t* __restrict__ sorted, const uint64_t* __restrict__ second, int64_t n, const uint8_t* __restrict__ head,
                                                             const int64_t* __restrict__ pos, uint64_t* __restrict__ ukeys, uint64_t* __restrict__ ukeys2, int64_t* __restrict__ start) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && head[i]) { ukeys[pos[i]] = sorted[i]; if (second) ukeys2[pos[i]] = second[i]; start[pos[i]] = i; }
  else if (i == n) start[pos[n]] = n;
}
// csum == nullptr: a segment's count is its length; else the sum of its counts, csum their exclusive prefix sums; *over: some sum passes 2^32 - 1
__global__ void __launch_bounds__(256) table_counts_kernel(const int64_t* __restrict__ start, int64_t n_seg, const uint64_t* __restrict__ csum, uint32_t* __restrict__ ucount,
                                                           unsigned long long* __restrict__ over) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= n_seg) return;
  const uint64_t s = csum ? csum[start[u + 1]] - csum[start[u]] : (uint64_t)(start[u + 1] - start[u]);
  ucount[u] = (uint32_t)s;
  if (s > 0xFFFFFFFFull) atomicMin(over, (unsigned long long)u);
}
__global__ void __launch_bounds__(256) interval_keys_kernel(const int32_t* __restrict__ contig, const int64_t* __restrict__ first, const int64_t* __restrict__ last, int64_t n,
                                                            uint64_t* __restrict__ skey, uint64_t* __restrict__ ekey) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { skey[i] = mmp::interval_key(contig[i], first[i]); ekey[i] = mmp::interval_key(contig[i], last[i]); }
}
// the depth at a row's contig and position (both key formats hold them in w0) and whether the thresholds keep the row; keep[n] = 0 for the scan's total
__global__ void __launch_bounds__(256) table_depth_kernel(const uint64_t* __restrict__ w0, const uint32_t* __restrict__ counts, int64_t n, const uint64_t* __restrict__ starts,
                                                          const uint64_t* __restrict__ ends, int64_t n_iv, int64_t min_count, double min_frac, uint32_t* __restrict__ depth,
                                                          uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int64_t d = mmp::depth_at(starts, ends, n_iv, mmp::key_contig(w0[i]), mmp::key_pos(w0[i]));
    depth[i] = (uint32_t)d;
    keep[i] = mmp::site_kept(counts[i], d, min_count, min_frac) ? 1 : 0;
  } else if (i == n) keep[i] = 0;
}

namespace {
template <class T> void gather(const T* src, const uint32_t* idx, int64_t n, int64_t n_dst, T* dst, hipStream_t st) {
  table_gather_kernel<T><<<dim3(flat_grid(n_dst)), dim3(256), 0, st>>>(src, idx, n, n_dst, dst); MM_KERNEL_CHECK();
}}  // namespace

void sort_table(DBuf<uint8_t>& tmp, uint64_t* w0, uint64_t* w1, uint32_t* counts, int64_t n, int bits0, int bits1, hipStream_t st, SortedTable* s) {
  const size_t k = (size_t)n;
  s->w0.alloc(k);
  if (counts) s->counts.alloc(k + 1);
  if (!w1) {
    if (!counts) { sort_keys(tmp, w0, s->w0.p, k, 0, bits0, st); return; }
    MM_HIP(hipMemsetAsync(s->counts.p + k, 0, sizeof(uint32_t), st));   // ([n] = 0: the scan's total)
    sort_pairs(tmp, w0, s->w0.p, counts, s->counts.p, k, 0, bits0, st);
    return;
  }
  s->w1.alloc(k); s->perm.alloc(k); s->i1.alloc(k);
  fill_iota(s->perm.p, n, st);
  sort_pairs(tmp, w1, s->w0.p, s->perm.p, s->i1.p, k, 0, bits1, st);
  gather(w0, s->i1.p, n, n, s->w1.p, st);
  sort_pairs(tmp, s->w1.p, s->w0.p, s->i1.p, s->perm.p, k, 0, bits0, st);
  gather(w1, s->perm.p, n, n, s->w1.p, st);
  if (counts) gather(counts, s->perm.p, n, n + 1, s->counts.p, st);
}

bool reduce_sorted(DBuf<uint8_t>& tmp, const SortedTable& s, int64_t n, hipStream_t st, KeyTable* out) {
  const size_t k = (size_t)n;
  const uint64_t* const second = s.w1.p;
  DBuf<uint8_t> d_head(k + 1); DBuf<int64_t> d_pos(k + 1), d_start(k + 1); DBuf<uint64_t> d_ukeys(k), d_ukeys2(second ? k : 1), d_csum; DBuf<uint32_t> d_ucount(k);
  DBuf<unsigned long long> d_over(1);
  table_heads_kernel<<<dim3(flat_grid(n + 1)), dim3(256), 0, st>>>(s.w0.p, second, n, d_head.p); MM_KERNEL_CHECK();
  exclusive_scan(tmp, d_head.p, d_pos.p, k + 1, st);
  table_segments_kernel<<<dim3(flat_grid(n + 1)), dim3(256), 0, st>>>(s.w0.p, second, n, d_head.p, d_pos.p, d_ukeys.p, d_ukeys2.p, d_start.p); MM_KERNEL_CHECK();
  int64_t n_seg = 0;
  d_pos.download(&n_seg, 1, st, k);
  MM_HIP(mm::stream_sync(st));
  if (s.counts.p) { d_csum.alloc(k + 1); exclusive_scan(tmp, s.counts.p, d_csum.p, k + 1, st); }
  MM_HIP(hipMemsetAsync(d_over.p, 0xFF, sizeof(unsigned long long), st));
  table_counts_kernel<<<dim3(flat_grid(n_seg)), dim3(256), 0, st>>>(d_start.p, n_seg, d_csum.p, d_ucount.p, d_over.p); MM_KERNEL_CHECK();
  const unsigned long long over = d_over.to_host(st)[0];
  if (over != ~0ull) return false;
  out->w0 = d_ukeys.to_host(st, (size_t)n_seg);
  if (second) out->w1 = d_ukeys2.to_host(st, (size_t)n_seg);
  out->counts = d_ucount.to_host(st, (size_t)n_seg);
  return true;
}

void merge_run(mm_ctx* ctx, int64_t n, const uint64_t* w0, const uint64_t* w1, const uint32_t* counts, const char* who, const char* timing_env, KeyTable* out) {
  out->clear();
  if (n == 0) return;
  hipStream_t st = ctx->stream;
  StageClock<3> clk(getenv(timing_env) != nullptr, st);           // upload, sort, reduce
  const size_t k = (size_t)n;
  uint64_t top0 = 0, top1 = 0;                                     // (two-word keys in one pass: the two chains of maxima overlap, which a pass per word would not)
  if (w1) for (size_t i = 0; i < k; ++i) { top0 = std::max(top0, w0[i]); top1 = std::max(top1, w1[i]); }
  else for (size_t i = 0; i < k; ++i) top0 = std::max(top0, w0[i]);
  clk.start();
  DBuf<uint64_t> d_w0(k), d_w1(w1 ? k : 0); DBuf<uint32_t> d_counts(k); DBuf<uint8_t> tmp;
  d_w0.upload(w0, k, st); d_w1.upload(w1, w1 ? k : 0, st); d_counts.upload(counts, k, st);
  clk.stop(0);
  clk.start();
  SortedTable sorted;
  sort_table(tmp, d_w0.p, d_w1.p, d_counts.p, n, bits_for(top0), bits_for(top1), st, &sorted);
  clk.stop(1);
  clk.start();
  const bool ok = reduce_sorted(tmp, sorted, n, st, out);
  clk.stop(2);
  if (!ok) out->clear();
  MM_REQUIRE(ok, MM_ERR_ARG, std::string(who) + ": the counts of a key add up to more than 2^32 - 1");
  if (clk.on) fprintf(stderr, "%s merge: upload %.3f sort %.3f reduce %.3f ms; %lld pairs in, %zu out\n", timing_env, clk.ms[0], clk.ms[1], clk.ms[2], (long long)n, out->w0.size());
}

int contig_bits(int64_t n_contigs) { return bits_for((uint64_t)std::max<int64_t>(n_contigs - 1, 0)); }

// The interval keys of n > 0 alignments (host arrays) on the device: starts ascending with end_of[i] the end that belongs to starts[i], ends ascending.
void sorted_interval_keys(DBuf<uint8_t>& tmp, const FinishIn& in, int bits, hipStream_t st, SortedIntervals& iv) {
  const size_t v = (size_t)in.n_iv;
  DBuf<int32_t> d_c(v); DBuf<int64_t> d_f(v), d_l(v); DBuf<uint64_t> d_skey(v), d_ekey(v);
  d_c.upload(in.iv_contig, v, st); d_f.upload(in.iv_first, v, st); d_l.upload(in.iv_last, v, st);
  interval_keys_kernel<<<dim3(flat_grid(in.n_iv)), dim3(256), 0, st>>>(d_c.p, d_f.p, d_l.p, in.n_iv, d_skey.p, d_ekey.p); MM_KERNEL_CHECK();
  sort_pairs(tmp, d_skey.p, iv.starts.p, d_ekey.p, iv.end_of.p, v, 0, bits, st);
  sort_keys(tmp, d_ekey.p, iv.ends.p, v, 0, bits, st);
  MM_HIP(mm::stream_sync(st));                                     // (the buffers of this scope)
}

bool finish_kept(mm_ctx* ctx, const mm_seqset* ref, const FinishIn& in, const char* who, const std::function<void()>& check_keys, const std::function<void(const KeptDev&)>& compact,
                 StageClock<3>& clk, SortedIntervals* iv, KeptRows* out) {
  const std::string w(who);
  MM_REQUIRE(ref->frozen, MM_ERR_STATE, w + ": the reference is not uploaded");
  MM_REQUIRE(ref->ctx->device == ctx->device, MM_ERR_ARG, w + ": the reference lives on another device");
  MM_REQUIRE(ref->count() <= mmp::MAX_CONTIGS, MM_ERR_ARG, w + ": more than 2^29 contigs");
  MM_REQUIRE(in.min_count >= 0 && in.min_frac >= 0 && in.min_frac <= 1, MM_ERR_ARG, w + ": min_count is negative or min_frac lies outside [0, 1]");
  check_keys();
  for (int64_t i = 0; i < in.n_iv; ++i)                           // every later index is inside its array
    MM_REQUIRE(in.iv_contig[i] >= 0 && in.iv_contig[i] < ref->count() && in.iv_first[i] >= 0 && in.iv_first[i] <= in.iv_last[i] && in.iv_last[i] < ref->len[(size_t)in.iv_contig[i]],
               MM_ERR_ARG, w + ": interval " + std::to_string(i) + " is empty or lies outside its contig");
  out->w0.clear(); out->count.clear(); out->depth.clear();
  const size_t k = (size_t)in.n, v = (size_t)in.n_iv;
  if (k == 0 && (v == 0 || !iv)) return false;
  hipStream_t st = ctx->stream;
  DBuf<uint8_t> tmp;
  SortedIntervals own;
  if (!iv) iv = &own;

  clk.start();
  iv->starts.alloc(std::max<size_t>(v, 1)); iv->end_of.alloc(std::max<size_t>(v, 1)); iv->ends.alloc(std::max<size_t>(v, 1));
  if (v) sorted_interval_keys(tmp, in, 32 + contig_bits(ref->count()), st, *iv);
  clk.stop(0);

  clk.start();
  if (k) {
    DBuf<uint64_t> d_w0(k), d_o0(k); DBuf<uint32_t> d_counts(k), d_depth(k), d_ocount(k), d_odepth(k); DBuf<uint8_t> d_keep(k + 1); DBuf<int64_t> d_pos(k + 1);
    d_w0.upload(in.w0, k, st); d_counts.upload(in.counts, k, st);
    table_depth_kernel<<<dim3(flat_grid(in.n + 1)), dim3(256), 0, st>>>(d_w0.p, d_counts.p, in.n, iv->starts.p, iv->ends.p, in.n_iv, in.min_count, in.min_frac, d_depth.p, d_keep.p);
    MM_KERNEL_CHECK();
    exclusive_scan(tmp, d_keep.p, d_pos.p, k + 1, st);
    compact(KeptDev{in.n, d_w0.p, d_counts.p, d_depth.p, d_keep.p, d_pos.p, d_o0.p, d_ocount.p, d_odepth.p});
    int64_t kept = 0;
    d_pos.download(&kept, 1, st, k);
    MM_HIP(mm::stream_sync(st));
    out->w0 = d_o0.to_host(st, (size_t)kept); out->count = d_ocount.to_host(st, (size_t)kept); out->depth = d_odepth.to_host(st, (size_t)kept);
  }
  return true;                                                     // (stage 1 stays open for what the format fetches beside the rows)
}

}  // namespace mm
