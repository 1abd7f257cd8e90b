// The pileup of a run's alignments on the device (mm_pileup_events / _merge / _finish; mapDirectly --pileup; DESIGN.md section 1, "Pileup"; the
// definition: mm_pileup_core.hpp, the text the host test runs).
//   events   count    pile_count_kernel: one wavefront (a 64-thread workgroup) per job; the lanes stride over the runs, sum the job's events and apply the
//                     rules.  A job that breaks one puts (job << 4 | rule) into the error word with an atomic minimum; the host reads the word before
//                     anything else is launched.
//            scan     an exclusive scan of the counts (mm_prims.hpp) places every job's events.
//            emit     pile_emit_kernel: one wavefront per job over tiles of 64 runs; a wave scan of the run lengths gives each run its contig position,
//                     its read index and its place; a lane expands its own short run, the wavefront a run of more than 64 events.  Read bases come
//                     through EditSeq::byte on a set narrowed to the read.  Keys are stored as 8-byte words, nothing else is written.
//            reduce   one radix sort of the keys over the bits in use, head flags, a scan and a scatter of (key, run length): mm_ident.hip's compaction.
//   merge    sort_pairs of (key, count), the same heads, and the sums of the segments as differences of one 64-bit prefix sum of the counts.
//   finish   the intervals' start keys (with their ends) and end keys sorted; a site's depth from two binary searches; kept sites compacted with the
//            reference's byte; per contig the alignments, the summed lengths and the union's length (each interval adds what lies beyond the running
//            maximum of the ends before it, an inclusive max-scan) with 64-bit vector atomics.
// No kernel here waits for another workgroup; the only atomics are the error words' minimum and the per-contig sums.
// The lane policy, the job arrays, the reduction (reduce_sorted, over one- or two-word keys) and the interval sort are shared with mm_vcf.hip: mm_pileup_dev.hpp.
#include "mm_pileup.hpp"
#include "mm_pileup_core.hpp"
#include "mm_pileup_dev.hpp"
#include "mm_edit_seq.hpp"
#include "mm_prims.hpp"

namespace mm {

__global__ void __launch_bounds__(64) pile_count_kernel(const int32_t* __restrict__ q_len, int64_t n_reads, const int32_t* __restrict__ r_len, int64_t n_contigs, PileJobs J,
                                                        int64_t job0, int64_t* __restrict__ counts, unsigned long long* __restrict__ err) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n) return;
  PileWaveLanes p;
  int64_t events = 0;
  int rule = 0;
  if (J.use[job] && J.dist[job] >= 0)
    rule = mmp::count_job(p, J.read[job], n_reads, J.contig[job], n_contigs, J.strand[job], q_len, r_len, J.first[job], J.ops + J.op_off[job], J.op_off[job + 1] - J.op_off[job], &events);
  if (threadIdx.x == 0) {
    counts[job] = events;
    if (rule) atomicMin(err, (unsigned long long)job << 4 | (unsigned long long)rule);
  }
}
// the events of job to keys[off[job], off[job + 1]); a job without events (not used, not aligned, or all =) writes nothing
__global__ void __launch_bounds__(64) pile_emit_kernel(EditSeq Q, const uint64_t* __restrict__ q_base, const int32_t* __restrict__ q_len, PileJobs J, int64_t job0,
                                                       const int64_t* __restrict__ off, uint64_t* __restrict__ keys) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n || off[job + 1] == off[job]) return;
  PileWaveLanes p;
  const int32_t read = J.read[job];
  const uint64_t qg = q_base[read];
  const int64_t m = q_len[read];
  mmp::emit_job(p, PileBytes{Q.narrowed(qg, qg + (uint64_t)m), (int64_t)qg}, m, J.strand[job], J.contig[job], J.first[job], J.ops + J.op_off[job], J.op_off[job + 1] - J.op_off[job],
                keys + off[job]);
}

// head[i]: sorted[i] starts a segment of equal keys; head[n] = 0 for the scan's total.  A key is sorted[i], with `second` (mm_vcf.hip's two-word keys) the
// pair (sorted[i], second[i]).
__global__ void __launch_bounds__(256) pile_heads_kernel(const uint64_t* __restrict__ sorted, const uint64_t* __restrict__ second, int64_t n, uint8_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) head[i] = i == 0 || sorted[i] != sorted[i - 1] || (second && second[i] != second[i - 1]) ? 1 : 0;
  else if (i == n) head[i] = 0;
}
// the segments' keys and first indexes; start[number of segments] = n
__global__ void __launch_bounds__(256) pile_segments_kernel(const uint64_t* __restrict__ sorted, const uint64_t* __restrict__ second, int64_t n, const uint8_t* __restrict__ head,
                                                            const int64_t* __restrict__ pos, uint64_t* __restrict__ ukeys, uint64_t* __restrict__ ukeys2, int64_t* __restrict__ start) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && head[i]) { ukeys[pos[i]] = sorted[i]; if (second) ukeys2[pos[i]] = second[i]; start[pos[i]] = i; }
  else if (i == n) start[pos[n]] = n;
}
// csum == nullptr: a segment's count is its length; else the sum of its counts, csum their exclusive prefix sums; *over: some sum passes 2^32 - 1
__global__ void __launch_bounds__(256) pile_counts_kernel(const int64_t* __restrict__ start, int64_t n_seg, const uint64_t* __restrict__ csum, uint32_t* __restrict__ ucount,
                                                          unsigned long long* __restrict__ over) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= n_seg) return;
  const uint64_t s = csum ? csum[start[u + 1]] - csum[start[u]] : (uint64_t)(start[u + 1] - start[u]);
  ucount[u] = (uint32_t)s;
  if (s > 0xFFFFFFFFull) atomicMin(over, (unsigned long long)u);
}

__global__ void __launch_bounds__(256) pile_interval_keys_kernel(const int32_t* __restrict__ contig, const int64_t* __restrict__ first, const int64_t* __restrict__ last, int64_t n,
                                                                 uint64_t* __restrict__ skey, uint64_t* __restrict__ ekey) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { skey[i] = mmp::interval_key(contig[i], first[i]); ekey[i] = mmp::interval_key(contig[i], last[i]); }
}
__global__ void __launch_bounds__(256) pile_depth_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts, int64_t n, const uint64_t* __restrict__ starts,
                                                         const uint64_t* __restrict__ ends, int64_t n_iv, int64_t min_count, double min_frac, uint32_t* __restrict__ depth,
                                                         uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int64_t d = mmp::depth_at(starts, ends, n_iv, mmp::key_contig(keys[i]), mmp::key_pos(keys[i]));
    depth[i] = (uint32_t)d;
    keep[i] = mmp::site_kept(counts[i], d, min_count, min_frac) ? 1 : 0;
  } else if (i == n) keep[i] = 0;
}
__global__ void __launch_bounds__(256) pile_sites_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ depth, int64_t n,
                                                         const uint8_t* __restrict__ keep, const int64_t* __restrict__ pos, EditSeq R, const uint64_t* __restrict__ r_base,
                                                         uint64_t* __restrict__ okey, uint32_t* __restrict__ ocount, uint32_t* __restrict__ odepth, uint8_t* __restrict__ oref) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !keep[i]) return;
  const int64_t o = pos[i];
  okey[o] = keys[i]; ocount[o] = counts[i]; odepth[o] = depth[i];
  oref[o] = R.byte((int64_t)r_base[mmp::key_contig(keys[i])] + mmp::key_pos(keys[i]));
}
// the intervals sorted by start key: end[i] belongs to start[i], pmax[i] is the largest end of the intervals 0 .. i
__global__ void __launch_bounds__(256) pile_coverage_kernel(const uint64_t* __restrict__ start, const uint64_t* __restrict__ end, const uint64_t* __restrict__ pmax, int64_t n,
                                                            unsigned long long* __restrict__ alignments, unsigned long long* __restrict__ covered,
                                                            unsigned long long* __restrict__ sum_depth) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = i < n;
  const int64_t c = in ? (int64_t)(start[i] >> 32) : -1;
  unsigned long long one = in ? 1 : 0, len = in ? end[i] - start[i] + 1 : 0, gain = in ? (unsigned long long)mmp::covered_gain(start[i], end[i], i > 0, i > 0 ? pmax[i - 1] : 0) : 0;
  // the intervals lie in contig order: a wavefront whose intervals share a contig (nearly every one) adds its sums once, integer sums in any order
  const int64_t c0 = __shfl((long long)c, 0, 64);
  if (__all(!in || c == c0)) {
    for (int d = 32; d > 0; d >>= 1) { one += __shfl_xor(one, d, 64); len += __shfl_xor(len, d, 64); gain += __shfl_xor(gain, d, 64); }
    if ((threadIdx.x & 63) != 0 || c0 < 0) return;
  } else if (!in) return;
  atomicAdd(&alignments[c], one);
  atomicAdd(&sum_depth[c], len);
  if (gain) atomicAdd(&covered[c], gain);
}

void pile_offsets_check(const int64_t* off, int64_t n, const char* who) {
  bool ok = off[0] >= 0;
  for (int64_t i = 0; ok && i < n; ++i) ok = off[i] <= off[i + 1];
  MM_REQUIRE(ok, MM_ERR_ARG, std::string(who) + ": op_off does not start at 0 or more, or falls");
}

// The segments of equal keys of sorted[0, n), n > 0: their keys, and their counts — the segments' lengths, or with d_counts (in the order of sorted,
// n + 1 entries, the last one 0) the sums of their counts.  With `second` a key is the pair (sorted[i], second[i]) and keys2 gets the second words.
// Returns false where a sum passes 2^32 - 1.
bool reduce_sorted(DBuf<uint8_t>& tmp, const uint64_t* sorted, const uint64_t* second, const uint32_t* d_counts, int64_t n, hipStream_t st, std::vector<uint64_t>* keys,
                   std::vector<uint64_t>* keys2, std::vector<uint32_t>* counts) {
  const size_t k = (size_t)n;
  DBuf<uint8_t> d_head(k + 1); DBuf<int64_t> d_pos(k + 1), d_start(k + 1); DBuf<uint64_t> d_ukeys(k), d_ukeys2(second ? k : 1), d_csum; DBuf<uint32_t> d_ucount(k);
  DBuf<unsigned long long> d_over(1);
  pile_heads_kernel<<<dim3(flat_grid(n + 1)), dim3(256), 0, st>>>(sorted, second, n, d_head.p); MM_KERNEL_CHECK();
  exclusive_scan(tmp, d_head.p, d_pos.p, k + 1, st);
  pile_segments_kernel<<<dim3(flat_grid(n + 1)), dim3(256), 0, st>>>(sorted, second, n, d_head.p, d_pos.p, d_ukeys.p, d_ukeys2.p, d_start.p); MM_KERNEL_CHECK();
  int64_t n_seg = 0;
  d_pos.download(&n_seg, 1, st, k);
  MM_HIP(mm::stream_sync(st));
  if (d_counts) { d_csum.alloc(k + 1); exclusive_scan(tmp, d_counts, d_csum.p, k + 1, st); }
  MM_HIP(hipMemsetAsync(d_over.p, 0xFF, sizeof(unsigned long long), st));
  pile_counts_kernel<<<dim3(flat_grid(n_seg)), dim3(256), 0, st>>>(d_start.p, n_seg, d_counts ? d_csum.p : nullptr, d_ucount.p, d_over.p); MM_KERNEL_CHECK();
  const unsigned long long over = d_over.to_host(st)[0];
  if (over != PILE_NO_ERROR) return false;
  *keys = d_ukeys.to_host(st, (size_t)n_seg);
  if (second) *keys2 = d_ukeys2.to_host(st, (size_t)n_seg);
  *counts = d_ucount.to_host(st, (size_t)n_seg);
  return true;
}

// The interval keys of n > 0 alignments (host arrays) on the device: starts ascending with end_of[i] the end that belongs to starts[i], ends ascending.
void sorted_interval_keys(DBuf<uint8_t>& tmp, int64_t n, const int32_t* contig, const int64_t* first, const int64_t* last, int bits, hipStream_t st, DBuf<uint64_t>& starts,
                          DBuf<uint64_t>& end_of, DBuf<uint64_t>& ends) {
  const size_t v = (size_t)n;
  DBuf<int32_t> d_c(v); DBuf<int64_t> d_f(v), d_l(v); DBuf<uint64_t> d_skey(v), d_ekey(v);
  d_c.upload(contig, v, st); d_f.upload(first, v, st); d_l.upload(last, v, st);
  pile_interval_keys_kernel<<<dim3(flat_grid(n)), dim3(256), 0, st>>>(d_c.p, d_f.p, d_l.p, n, d_skey.p, d_ekey.p); MM_KERNEL_CHECK();
  sort_pairs(tmp, d_skey.p, starts.p, d_ekey.p, end_of.p, v, 0, bits, st);
  sort_keys(tmp, d_ekey.p, ends.p, v, 0, bits, st);
  MM_HIP(mm::stream_sync(st));                                     // (the buffers of this scope)
}
int contig_bits(int64_t n_contigs) { return bits_for((uint64_t)std::max<int64_t>(n_contigs - 1, 0)); }

void pileup_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const PileupIn& in, PileupTable* out) {
  MM_REQUIRE(reads->frozen && ref->frozen, MM_ERR_STATE, "mm_pileup_events: a sequence set is not uploaded");
  MM_REQUIRE(reads->ctx->device == ctx->device && ref->ctx->device == ctx->device, MM_ERR_ARG, "mm_pileup_events: a sequence set lives on another device");
  MM_REQUIRE(ref->count() <= mmp::MAX_CONTIGS, MM_ERR_ARG, "mm_pileup_events: more than 2^29 contigs");
  out->keys.clear(); out->counts.clear();
  const int64_t n = in.n_jobs;
  if (n == 0) return;
  pile_offsets_check(in.op_off, n, "mm_pileup_events");
  const size_t k = (size_t)n, n_ops = (size_t)in.op_off[n];
  MM_REQUIRE(n_ops == 0 || in.ops, MM_ERR_ARG, "mm_pileup_events: a null array");
  hipStream_t st = ctx->stream;
  StageClock<6> clk(getenv("MM_PILEUP_TIMING") != nullptr, st);    // upload, count, scan, emit, sort, reduce (with the table's way to the host)

  clk.start();
  DBuf<int32_t> d_read(k), d_strand(k), d_contig(k), d_dist(k);
  DBuf<int64_t> d_first(k), d_op_off(k + 1), d_counts(k + 1), d_off(k + 1);
  DBuf<uint32_t> d_ops(std::max<size_t>(n_ops, 1));
  DBuf<uint8_t> d_use(k);
  DBuf<unsigned long long> d_err(1);
  d_read.upload(in.read, k, st); d_strand.upload(in.strand, k, st); d_contig.upload(in.contig, k, st); d_dist.upload(in.dist, k, st); d_first.upload(in.first, k, st);
  d_op_off.upload(in.op_off, k + 1, st); d_ops.upload(in.ops, n_ops, st); d_use.upload(in.use, k, st);
  d_counts.zero(st);
  MM_HIP(hipMemsetAsync(d_err.p, 0xFF, sizeof(unsigned long long), st));
  clk.stop(0);
  const PileJobs J{n, d_read.p, d_strand.p, d_contig.p, d_dist.p, d_first.p, d_op_off.p, d_ops.p, d_use.p};

  clk.start();
  for (int64_t job0 = 0; job0 < n; job0 += PILE_GRID_MAX) {
    pile_count_kernel<<<dim3((unsigned)std::min(PILE_GRID_MAX, n - job0)), dim3(64), 0, st>>>(reads->d_len.p, reads->count(), ref->d_len.p, ref->count(), J, job0, d_counts.p, d_err.p);
    MM_KERNEL_CHECK();
  }
  const unsigned long long e = d_err.to_host(st)[0];
  clk.stop(1);
  MM_REQUIRE(e == PILE_NO_ERROR, MM_ERR_ARG, "mm_pileup_events: job " + std::to_string(e >> 4) + ": " + mmp::rule_text((int)(e & 15)));

  clk.start();
  DBuf<uint8_t> tmp;
  exclusive_scan(tmp, d_counts.p, d_off.p, k + 1, st);
  int64_t total = 0;
  d_off.download(&total, 1, st, k);
  MM_HIP(mm::stream_sync(st));
  clk.stop(2);
  MM_REQUIRE(total < ((int64_t)1 << 32), MM_ERR_LIMIT, "mm_pileup_events: 2^32 events or more in one call");
  if (total > 0) {
    clk.start();
    DBuf<uint64_t> d_keys((size_t)total), d_sorted((size_t)total);
    for (int64_t job0 = 0; job0 < n; job0 += PILE_GRID_MAX) {
      pile_emit_kernel<<<dim3((unsigned)std::min(PILE_GRID_MAX, n - job0)), dim3(64), 0, st>>>(edit_seq(reads), reads->d_base.p, reads->d_len.p, J, job0, d_off.p, d_keys.p);
      MM_KERNEL_CHECK();
    }
    clk.stop(3);
    clk.start();
    sort_keys(tmp, d_keys.p, d_sorted.p, (size_t)total, 0, mmp::CONTIG_SHIFT + contig_bits(ref->count()), st);
    clk.stop(4);
    clk.start();
    reduce_sorted(tmp, d_sorted.p, nullptr, nullptr, total, st, &out->keys, nullptr, &out->counts);
    clk.stop(5);
  }
  if (clk.on)
    fprintf(stderr, "MM_PILEUP_TIMING events: upload %.3f count %.3f scan %.3f emit %.3f sort %.3f reduce %.3f ms; %lld jobs, %lld runs, %lld events, %zu pairs, %zu B fetched\n", clk.ms[0],
            clk.ms[1], clk.ms[2], clk.ms[3], clk.ms[4], clk.ms[5], (long long)n, (long long)n_ops, (long long)total, out->keys.size(), out->keys.size() * 12);
}

void pileup_merge_run(mm_ctx* ctx, int64_t n, const uint64_t* keys, const uint32_t* counts, PileupTable* out) {
  out->keys.clear(); out->counts.clear();
  if (n == 0) return;
  hipStream_t st = ctx->stream;
  StageClock<3> clk(getenv("MM_PILEUP_TIMING") != nullptr, st);    // upload, sort, reduce
  const size_t k = (size_t)n;
  uint64_t top = 0;
  for (size_t i = 0; i < k; ++i) top = std::max(top, keys[i]);
  clk.start();
  DBuf<uint64_t> d_keys(k), d_sorted(k); DBuf<uint32_t> d_counts(k), d_csorted(k + 1); DBuf<uint8_t> tmp;
  d_keys.upload(keys, k, st); d_counts.upload(counts, k, st);
  d_csorted.zero(st);                                              // ([n] stays 0: the scan's total)
  clk.stop(0);
  clk.start();
  sort_pairs(tmp, d_keys.p, d_sorted.p, d_counts.p, d_csorted.p, k, 0, bits_for(top), st);
  clk.stop(1);
  clk.start();
  const bool ok = reduce_sorted(tmp, d_sorted.p, nullptr, d_csorted.p, n, st, &out->keys, nullptr, &out->counts);
  clk.stop(2);
  if (!ok) { out->keys.clear(); out->counts.clear(); }
  MM_REQUIRE(ok, MM_ERR_ARG, "mm_pileup_merge: the counts of a key add up to more than 2^32 - 1");
  if (clk.on) fprintf(stderr, "MM_PILEUP_TIMING merge: upload %.3f sort %.3f reduce %.3f ms; %lld pairs in, %zu out\n", clk.ms[0], clk.ms[1], clk.ms[2], (long long)n, out->keys.size());
}

namespace {
// what mm_pileup_finish asks of its arrays before anything is launched: every later index is inside its array
void finish_check(const mm_seqset* ref, const PileupFinishIn& in) {
  const int64_t nc = ref->count();
  for (int64_t i = 0; i < in.n; ++i) {
    const uint64_t key = in.keys[i];
    MM_REQUIRE(i == 0 || in.keys[i - 1] < key, MM_ERR_ARG, "mm_pileup_finish: the keys are not ascending and unique (entry " + std::to_string(i) + "): pass a merged table");
    MM_REQUIRE(mmp::key_contig(key) < nc && mmp::key_pos(key) < ref->len[(size_t)mmp::key_contig(key)] && mmp::key_code(key) < mmp::N_CODES, MM_ERR_ARG,
               "mm_pileup_finish: entry " + std::to_string(i) + " names no position of the reference, or no code");
  }
  for (int64_t i = 0; i < in.n_iv; ++i)
    MM_REQUIRE(in.iv_contig[i] >= 0 && in.iv_contig[i] < nc && in.iv_first[i] >= 0 && in.iv_first[i] <= in.iv_last[i] && in.iv_last[i] < ref->len[(size_t)in.iv_contig[i]], MM_ERR_ARG,
               "mm_pileup_finish: interval " + std::to_string(i) + " is empty or lies outside its contig");
}
}  // namespace

void pileup_finish_run(mm_ctx* ctx, const mm_seqset* ref, const PileupFinishIn& in, PileupResult* out) {
  MM_REQUIRE(ref->frozen, MM_ERR_STATE, "mm_pileup_finish: the reference is not uploaded");
  MM_REQUIRE(ref->ctx->device == ctx->device, MM_ERR_ARG, "mm_pileup_finish: the reference lives on another device");
  MM_REQUIRE(ref->count() <= mmp::MAX_CONTIGS, MM_ERR_ARG, "mm_pileup_finish: more than 2^29 contigs");
  MM_REQUIRE(in.min_count >= 0 && in.min_frac >= 0 && in.min_frac <= 1, MM_ERR_ARG, "mm_pileup_finish: min_count is negative or min_frac lies outside [0, 1]");
  finish_check(ref, in);
  const size_t nc = (size_t)ref->count(), k = (size_t)in.n, v = (size_t)in.n_iv;
  out->key.clear(); out->count.clear(); out->depth.clear(); out->ref_byte.clear();
  out->alignments.assign(nc, 0); out->covered.assign(nc, 0); out->sum_depth.assign(nc, 0);
  if (nc == 0 || (k == 0 && v == 0)) return;
  hipStream_t st = ctx->stream;
  StageClock<3> clk(getenv("MM_PILEUP_TIMING") != nullptr, st);    // intervals (upload and sorts), sites, coverage
  DBuf<uint8_t> tmp;
  const int bits = 32 + contig_bits(ref->count());

  clk.start();
  DBuf<uint64_t> d_starts(std::max<size_t>(v, 1)), d_end_of(std::max<size_t>(v, 1)), d_ends(std::max<size_t>(v, 1));
  if (v) sorted_interval_keys(tmp, in.n_iv, in.iv_contig, in.iv_first, in.iv_last, bits, st, d_starts, d_end_of, d_ends);
  clk.stop(0);

  clk.start();
  if (k) {
    DBuf<uint64_t> d_keys(k), d_okey(k); DBuf<uint32_t> d_counts(k), d_depth(k), d_ocount(k), d_odepth(k); DBuf<uint8_t> d_keep(k + 1), d_oref(k); DBuf<int64_t> d_pos(k + 1);
    d_keys.upload(in.keys, k, st); d_counts.upload(in.counts, k, st);
    pile_depth_kernel<<<dim3(flat_grid(in.n + 1)), dim3(256), 0, st>>>(d_keys.p, d_counts.p, in.n, d_starts.p, d_ends.p, in.n_iv, in.min_count, in.min_frac, d_depth.p, d_keep.p);
    MM_KERNEL_CHECK();
    exclusive_scan(tmp, d_keep.p, d_pos.p, k + 1, st);
    pile_sites_kernel<<<dim3(flat_grid(in.n)), dim3(256), 0, st>>>(d_keys.p, d_counts.p, d_depth.p, in.n, d_keep.p, d_pos.p, edit_seq(ref), ref->d_base.p, d_okey.p, d_ocount.p,
                                                                   d_odepth.p, d_oref.p);
    MM_KERNEL_CHECK();
    int64_t kept = 0;
    d_pos.download(&kept, 1, st, k);
    MM_HIP(mm::stream_sync(st));
    out->key = d_okey.to_host(st, (size_t)kept); out->count = d_ocount.to_host(st, (size_t)kept);
    out->depth = d_odepth.to_host(st, (size_t)kept); out->ref_byte = d_oref.to_host(st, (size_t)kept);
  }
  clk.stop(1);

  clk.start();
  if (v) {
    DBuf<uint64_t> d_pmax(v); DBuf<unsigned long long> d_sums(3 * nc);
    d_sums.zero(st);
    with_scratch(tmp, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, d_end_of.p, d_pmax.p, v, rocprim::maximum<uint64_t>(), st); });
    pile_coverage_kernel<<<dim3(flat_grid(in.n_iv)), dim3(256), 0, st>>>(d_starts.p, d_end_of.p, d_pmax.p, in.n_iv, d_sums.p, d_sums.p + nc, d_sums.p + 2 * nc); MM_KERNEL_CHECK();
    const std::vector<unsigned long long> s = d_sums.to_host(st);
    for (size_t c = 0; c < nc; ++c) { out->alignments[c] = (int64_t)s[c]; out->covered[c] = (int64_t)s[nc + c]; out->sum_depth[c] = (int64_t)s[2 * nc + c]; }
  }
  clk.stop(2);
  if (clk.on)
    fprintf(stderr, "MM_PILEUP_TIMING finish: intervals %.3f sites %.3f coverage %.3f ms; %lld entries, %lld intervals, %zu sites kept\n", clk.ms[0], clk.ms[1], clk.ms[2], (long long)in.n,
            (long long)in.n_iv, out->key.size());
}

}  // namespace mm
