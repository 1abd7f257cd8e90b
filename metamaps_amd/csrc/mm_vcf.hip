// The alleles of a run's alignments on the device (mm_vcf_events / _merge / _finish; mapDirectly --vcf; DESIGN.md section 1, "VCF"; the definition:
// mm_vcf_core.hpp, the text the host test runs).
//   events   count    vcf_count_kernel: one wavefront (a 64-thread workgroup) per job; the lanes stride over the runs, apply the rules and sum the job's bound of
//                     alleles (X bases + the I and D runs between other runs) and its indel runs.  A job that breaks a rule puts (job << 4 | rule) into the
//                     error word with an atomic minimum; the host reads the word before anything else is launched.
//            scan     exclusive scans of the two counts (mm_prims.hpp): every job's place, and whether the call has an indel at all.
//            emit     vcf_emit_kernel: one wavefront per job over tiles of 64 runs; wave scans give each run its contig position, its read index and its
//                     place; a lane writes its own short run and left-aligns its own indel (a loop of at most NORM_MAX steps over EditSeq::byte on the
//                     job's contig, no shuffle inside), the wavefront expands an X run of more than 64 bases.  A skipped event is the all-ones pair.
//            sort     two stable radix passes over an index: by w1 (skipped when the call has no indel: every w1 is 0 or all ones), then by the bits of w0
//                     in use.  The all-ones pairs sort last and are cut off the table.
//            reduce   mm_pileup.hip's heads, scan, scatter and counts over two-word keys.
//   merge    the same two passes with the counts gathered behind the index, and the sums of the segments from one 64-bit prefix sum.
//   finish   the intervals' start and end keys sorted (mm_pileup.hip); an allele's depth from two binary searches; kept alleles compacted with their
//            reference windows.
// No kernel here waits for another workgroup; the only atomics are the error words' minimum.
#include "mm_vcf.hpp"
#include "mm_vcf_core.hpp"
#include "mm_pileup_dev.hpp"
#include "mm_prims.hpp"

namespace mm {

__global__ void __launch_bounds__(64) vcf_count_kernel(const int32_t* __restrict__ q_len, int64_t n_reads, const int32_t* __restrict__ r_len, int64_t n_contigs, PileJobs J,
                                                       int64_t job0, int64_t* __restrict__ counts, int64_t* __restrict__ indels, unsigned long long* __restrict__ err) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n) return;
  PileWaveLanes p;
  int64_t alleles = 0, ind = 0;
  int rule = 0;
  if (J.use[job] && J.dist[job] >= 0)
    rule = mmv::count_job(p, J.read[job], n_reads, J.contig[job], n_contigs, J.strand[job], q_len, r_len, J.first[job], J.ops + J.op_off[job], J.op_off[job + 1] - J.op_off[job], &alleles,
                          &ind);
  if (threadIdx.x == 0) {
    counts[job] = alleles; indels[job] = ind;
    if (rule) atomicMin(err, (unsigned long long)job << 4 | (unsigned long long)rule);
  }
}
// the alleles of job to w0 and w1 [off[job], off[job + 1]); a job without any (not used, not aligned, or nothing but = and edge runs) writes nothing
__global__ void __launch_bounds__(64) vcf_emit_kernel(EditSeq Q, const uint64_t* __restrict__ q_base, const int32_t* __restrict__ q_len, EditSeq R, const uint64_t* __restrict__ r_base,
                                                      PileJobs J, int64_t job0, const int64_t* __restrict__ off, uint64_t* __restrict__ w0, uint64_t* __restrict__ w1) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n || off[job + 1] == off[job]) return;
  PileWaveLanes p;
  const int32_t read = J.read[job], contig = J.contig[job];
  const uint64_t qg = q_base[read];
  const int64_t m = q_len[read];
  mmv::emit_job(p, PileBytes{Q.narrowed(qg, qg + (uint64_t)m), (int64_t)qg}, m, J.strand[job], PileBytes{R, (int64_t)r_base[contig]}, contig, J.first[job], J.ops + J.op_off[job],
                J.op_off[job + 1] - J.op_off[job], w0 + off[job], w1 + off[job]);
}

// dst[i] = src[idx[i]] for i < n; dst[n .. n_dst) = 0 (the counts' last entry: the scan's total)
template <class T> __global__ void __launch_bounds__(256) vcf_gather_kernel(const T* __restrict__ src, const uint32_t* __restrict__ idx, int64_t n, int64_t n_dst, T* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
  else if (i < n_dst) dst[i] = 0;
}
__global__ void __launch_bounds__(256) vcf_depth_kernel(const uint64_t* __restrict__ w0, const uint32_t* __restrict__ counts, int64_t n, const uint64_t* __restrict__ starts,
                                                        const uint64_t* __restrict__ ends, int64_t n_iv, int64_t min_count, double min_frac, uint32_t* __restrict__ depth,
                                                        uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int64_t d = mmp::depth_at(starts, ends, n_iv, mmp::key_contig(w0[i]), mmp::key_pos(w0[i]));
    depth[i] = (uint32_t)d;
    keep[i] = mmp::site_kept(counts[i], d, min_count, min_frac) ? 1 : 0;
  } else if (i == n) keep[i] = 0;
}
// a kept allele to its place pos[i], with the reference's bytes from its position on (zero beyond the contig's end)
__global__ void __launch_bounds__(256) vcf_alleles_kernel(const uint64_t* __restrict__ w0, const uint64_t* __restrict__ w1, const uint32_t* __restrict__ counts,
                                                          const uint32_t* __restrict__ depth, int64_t n, const uint8_t* __restrict__ keep, const int64_t* __restrict__ pos, EditSeq R,
                                                          const uint64_t* __restrict__ r_base, const int32_t* __restrict__ r_len, uint64_t* __restrict__ o0, uint64_t* __restrict__ o1,
                                                          uint32_t* __restrict__ ocount, uint32_t* __restrict__ odepth, uint8_t* __restrict__ owin) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !keep[i]) return;
  const int64_t o = pos[i], c = mmp::key_contig(w0[i]), at = mmp::key_pos(w0[i]);
  o0[o] = w0[i]; o1[o] = w1[i]; ocount[o] = counts[i]; odepth[o] = depth[i];
  const int64_t len = mmv::window_len(at, r_len[c]);
  for (int64_t t = 0; t < mmv::WINDOW; ++t) owin[o * mmv::WINDOW + t] = t < len ? R.byte((int64_t)r_base[c] + at + t) : (uint8_t)0;
}

namespace {
template <class T> void gather(const T* src, const uint32_t* idx, int64_t n, int64_t n_dst, T* dst, hipStream_t st) {
  vcf_gather_kernel<T><<<dim3(flat_grid(n_dst)), dim3(256), 0, st>>>(src, idx, n, n_dst, dst); MM_KERNEL_CHECK();
}
// The order of the two-word keys (w0[i], w1[i]), i < n < 2^32, by two stable passes over an index: by bits [0, bits1) of w1, then by bits [0, bits0) of w0.
// Leaves the sorted w0 in a, their w1 in b and the index of every sorted key in perm; i1 is scratch.  All buffers hold n entries.
void sort_two_words(DBuf<uint8_t>& tmp, uint64_t* w0, uint64_t* w1, int64_t n, int bits0, int bits1, hipStream_t st, uint64_t* a, uint64_t* b, uint32_t* perm, uint32_t* i1) {
  fill_iota(perm, n, st);
  sort_pairs(tmp, w1, a, perm, i1, (size_t)n, 0, bits1, st);
  gather(w0, i1, n, n, b, st);
  sort_pairs(tmp, b, a, i1, perm, (size_t)n, 0, bits0, st);
  gather(w1, perm, n, n, b, st);
}
void cut_skipped(VcfTable* t) {                                   // the all-ones pair, the last segment where there is one, is no allele
  if (!t->w0.empty() && t->w0.back() == mmv::SKIP) { t->w0.pop_back(); t->w1.pop_back(); t->counts.pop_back(); }
}
}  // namespace

void vcf_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const PileupIn& in, VcfTable* out) {
  MM_REQUIRE(reads->frozen && ref->frozen, MM_ERR_STATE, "mm_vcf_events: a sequence set is not uploaded");
  MM_REQUIRE(reads->ctx->device == ctx->device && ref->ctx->device == ctx->device, MM_ERR_ARG, "mm_vcf_events: a sequence set lives on another device");
  MM_REQUIRE(ref->count() <= mmp::MAX_CONTIGS, MM_ERR_ARG, "mm_vcf_events: more than 2^29 contigs");
  out->w0.clear(); out->w1.clear(); out->counts.clear();
  const int64_t n = in.n_jobs;
  if (n == 0) return;
  pile_offsets_check(in.op_off, n, "mm_vcf_events");
  const size_t k = (size_t)n, n_ops = (size_t)in.op_off[n];
  MM_REQUIRE(n_ops == 0 || in.ops, MM_ERR_ARG, "mm_vcf_events: a null array");
  hipStream_t st = ctx->stream;
  StageClock<6> clk(getenv("MM_VCF_TIMING") != nullptr, st);       // upload, count, scan, emit, sort, reduce (with the table's way to the host)

  clk.start();
  DBuf<int32_t> d_read(k), d_strand(k), d_contig(k), d_dist(k);
  DBuf<int64_t> d_first(k), d_op_off(k + 1), d_counts(k + 1), d_indels(k + 1), d_off(k + 1), d_ioff(k + 1);
  DBuf<uint32_t> d_ops(std::max<size_t>(n_ops, 1));
  DBuf<uint8_t> d_use(k);
  DBuf<unsigned long long> d_err(1);
  d_read.upload(in.read, k, st); d_strand.upload(in.strand, k, st); d_contig.upload(in.contig, k, st); d_dist.upload(in.dist, k, st); d_first.upload(in.first, k, st);
  d_op_off.upload(in.op_off, k + 1, st); d_ops.upload(in.ops, n_ops, st); d_use.upload(in.use, k, st);
  d_counts.zero(st); d_indels.zero(st);
  MM_HIP(hipMemsetAsync(d_err.p, 0xFF, sizeof(unsigned long long), st));
  clk.stop(0);
  const PileJobs J{n, d_read.p, d_strand.p, d_contig.p, d_dist.p, d_first.p, d_op_off.p, d_ops.p, d_use.p};

  clk.start();
  for (int64_t job0 = 0; job0 < n; job0 += PILE_GRID_MAX) {
    vcf_count_kernel<<<dim3((unsigned)std::min(PILE_GRID_MAX, n - job0)), dim3(64), 0, st>>>(reads->d_len.p, reads->count(), ref->d_len.p, ref->count(), J, job0, d_counts.p, d_indels.p,
                                                                                             d_err.p);
    MM_KERNEL_CHECK();
  }
  const unsigned long long e = d_err.to_host(st)[0];
  clk.stop(1);
  MM_REQUIRE(e == PILE_NO_ERROR, MM_ERR_ARG, "mm_vcf_events: job " + std::to_string(e >> 4) + ": " + mmv::rule_text((int)(e & 15)));

  clk.start();
  DBuf<uint8_t> tmp;
  exclusive_scan(tmp, d_counts.p, d_off.p, k + 1, st);
  exclusive_scan(tmp, d_indels.p, d_ioff.p, k + 1, st);
  int64_t total = 0, indels = 0;
  d_off.download(&total, 1, st, k);
  d_ioff.download(&indels, 1, st, k);
  MM_HIP(mm::stream_sync(st));
  clk.stop(2);
  MM_REQUIRE(total < ((int64_t)1 << 32), MM_ERR_LIMIT, "mm_vcf_events: 2^32 events or more in one call");
  if (total > 0) {
    clk.start();
    const size_t t = (size_t)total;
    DBuf<uint64_t> d_w0(t), d_w1(t), d_a(t), d_b;
    for (int64_t job0 = 0; job0 < n; job0 += PILE_GRID_MAX) {
      vcf_emit_kernel<<<dim3((unsigned)std::min(PILE_GRID_MAX, n - job0)), dim3(64), 0, st>>>(edit_seq(reads), reads->d_base.p, reads->d_len.p, edit_seq(ref), ref->d_base.p, J, job0,
                                                                                              d_off.p, d_w0.p, d_w1.p);
      MM_KERNEL_CHECK();
    }
    clk.stop(3);
    clk.start();
    const int bits0 = mmp::CONTIG_SHIFT + contig_bits(ref->count());
    if (indels) {
      DBuf<uint32_t> d_perm(t), d_i1(t);
      d_b.alloc(t);
      sort_two_words(tmp, d_w0.p, d_w1.p, total, bits0, 64, st, d_a.p, d_b.p, d_perm.p, d_i1.p);
      MM_HIP(mm::stream_sync(st));                                 // (the two index buffers of this scope)
    } else sort_keys(tmp, d_w0.p, d_a.p, t, 0, bits0, st);         // every w1 is 0, or all ones beside an all-ones w0
    clk.stop(4);
    clk.start();
    reduce_sorted(tmp, d_a.p, indels ? d_b.p : nullptr, nullptr, total, st, &out->w0, &out->w1, &out->counts);
    if (!indels) out->w1.assign(out->w0.size(), 0);
    cut_skipped(out);
    clk.stop(5);
  }
  if (clk.on)
    fprintf(stderr, "MM_VCF_TIMING events: upload %.3f count %.3f scan %.3f emit %.3f sort %.3f reduce %.3f ms; %lld jobs, %lld runs, %lld events (%lld indels), %zu pairs, %zu B fetched\n",
            clk.ms[0], clk.ms[1], clk.ms[2], clk.ms[3], clk.ms[4], clk.ms[5], (long long)n, (long long)n_ops, (long long)total, (long long)indels, out->w0.size(), out->w0.size() * 20);
}

void vcf_merge_run(mm_ctx* ctx, int64_t n, const uint64_t* w0, const uint64_t* w1, const uint32_t* counts, VcfTable* out) {
  out->w0.clear(); out->w1.clear(); out->counts.clear();
  if (n == 0) return;
  hipStream_t st = ctx->stream;
  StageClock<3> clk(getenv("MM_VCF_TIMING") != nullptr, st);       // upload, sort, reduce
  const size_t k = (size_t)n;
  uint64_t top0 = 0, top1 = 0;
  for (size_t i = 0; i < k; ++i) { top0 = std::max(top0, w0[i]); top1 = std::max(top1, w1[i]); }
  clk.start();
  DBuf<uint64_t> d_w0(k), d_w1(k), d_a(k), d_b(k); DBuf<uint32_t> d_counts(k), d_csorted(k + 1), d_perm(k), d_i1(k); DBuf<uint8_t> tmp;
  d_w0.upload(w0, k, st); d_w1.upload(w1, k, st); d_counts.upload(counts, k, st);
  clk.stop(0);
  clk.start();
  sort_two_words(tmp, d_w0.p, d_w1.p, n, bits_for(top0), bits_for(top1), st, d_a.p, d_b.p, d_perm.p, d_i1.p);
  gather(d_counts.p, d_perm.p, n, n + 1, d_csorted.p, st);         // ([n] = 0: the scan's total)
  clk.stop(1);
  clk.start();
  const bool ok = reduce_sorted(tmp, d_a.p, d_b.p, d_csorted.p, n, st, &out->w0, &out->w1, &out->counts);
  clk.stop(2);
  if (!ok) { out->w0.clear(); out->w1.clear(); out->counts.clear(); }
  MM_REQUIRE(ok, MM_ERR_ARG, "mm_vcf_merge: the counts of a key add up to more than 2^32 - 1");
  if (clk.on) fprintf(stderr, "MM_VCF_TIMING merge: upload %.3f sort %.3f reduce %.3f ms; %lld pairs in, %zu out\n", clk.ms[0], clk.ms[1], clk.ms[2], (long long)n, out->w0.size());
}

namespace {
// what mm_vcf_finish asks of its arrays before anything is launched: every later index is inside its array
void finish_check(const mm_seqset* ref, const VcfFinishIn& in) {
  const int64_t nc = ref->count();
  for (int64_t i = 0; i < in.n; ++i) {
    const uint64_t a = in.w0[i], b = in.w1[i];
    MM_REQUIRE(i == 0 || in.w0[i - 1] < a || (in.w0[i - 1] == a && in.w1[i - 1] < b), MM_ERR_ARG,
               "mm_vcf_finish: the keys are not ascending and unique (entry " + std::to_string(i) + "): pass a merged table");
    MM_REQUIRE(mmp::key_contig(a) < nc && mmv::key_valid(a, b, ref->len[(size_t)mmp::key_contig(a)]), MM_ERR_ARG,
               "mm_vcf_finish: entry " + std::to_string(i) + " names no position of the reference, or no allele");
  }
  for (int64_t i = 0; i < in.n_iv; ++i)
    MM_REQUIRE(in.iv_contig[i] >= 0 && in.iv_contig[i] < nc && in.iv_first[i] >= 0 && in.iv_first[i] <= in.iv_last[i] && in.iv_last[i] < ref->len[(size_t)in.iv_contig[i]], MM_ERR_ARG,
               "mm_vcf_finish: interval " + std::to_string(i) + " is empty or lies outside its contig");
}
}  // namespace

void vcf_finish_run(mm_ctx* ctx, const mm_seqset* ref, const VcfFinishIn& in, VcfResult* out) {
  MM_REQUIRE(ref->frozen, MM_ERR_STATE, "mm_vcf_finish: the reference is not uploaded");
  MM_REQUIRE(ref->ctx->device == ctx->device, MM_ERR_ARG, "mm_vcf_finish: the reference lives on another device");
  MM_REQUIRE(ref->count() <= mmp::MAX_CONTIGS, MM_ERR_ARG, "mm_vcf_finish: more than 2^29 contigs");
  MM_REQUIRE(in.min_count >= 0 && in.min_frac >= 0 && in.min_frac <= 1, MM_ERR_ARG, "mm_vcf_finish: min_count is negative or min_frac lies outside [0, 1]");
  finish_check(ref, in);
  out->w0.clear(); out->w1.clear(); out->count.clear(); out->depth.clear(); out->window.clear();
  const size_t k = (size_t)in.n, v = (size_t)in.n_iv;
  if (k == 0) return;
  hipStream_t st = ctx->stream;
  StageClock<2> clk(getenv("MM_VCF_TIMING") != nullptr, st);       // intervals (upload and sorts), alleles
  DBuf<uint8_t> tmp;

  clk.start();
  DBuf<uint64_t> d_starts(std::max<size_t>(v, 1)), d_end_of(std::max<size_t>(v, 1)), d_ends(std::max<size_t>(v, 1));
  if (v) sorted_interval_keys(tmp, in.n_iv, in.iv_contig, in.iv_first, in.iv_last, 32 + contig_bits(ref->count()), st, d_starts, d_end_of, d_ends);
  clk.stop(0);

  clk.start();
  DBuf<uint64_t> d_w0(k), d_w1(k), d_o0(k), d_o1(k); DBuf<uint32_t> d_counts(k), d_depth(k), d_ocount(k), d_odepth(k); DBuf<uint8_t> d_keep(k + 1), d_owin(k * mmv::WINDOW);
  DBuf<int64_t> d_pos(k + 1);
  d_w0.upload(in.w0, k, st); d_w1.upload(in.w1, k, st); d_counts.upload(in.counts, k, st);
  vcf_depth_kernel<<<dim3(flat_grid(in.n + 1)), dim3(256), 0, st>>>(d_w0.p, d_counts.p, in.n, d_starts.p, d_ends.p, in.n_iv, in.min_count, in.min_frac, d_depth.p, d_keep.p);
  MM_KERNEL_CHECK();
  exclusive_scan(tmp, d_keep.p, d_pos.p, k + 1, st);
  vcf_alleles_kernel<<<dim3(flat_grid(in.n)), dim3(256), 0, st>>>(d_w0.p, d_w1.p, d_counts.p, d_depth.p, in.n, d_keep.p, d_pos.p, edit_seq(ref), ref->d_base.p, ref->d_len.p, d_o0.p,
                                                                  d_o1.p, d_ocount.p, d_odepth.p, d_owin.p);
  MM_KERNEL_CHECK();
  int64_t kept = 0;
  d_pos.download(&kept, 1, st, k);
  MM_HIP(mm::stream_sync(st));
  out->w0 = d_o0.to_host(st, (size_t)kept); out->w1 = d_o1.to_host(st, (size_t)kept);
  out->count = d_ocount.to_host(st, (size_t)kept); out->depth = d_odepth.to_host(st, (size_t)kept); out->window = d_owin.to_host(st, (size_t)kept * mmv::WINDOW);
  clk.stop(1);
  if (clk.on)
    fprintf(stderr, "MM_VCF_TIMING finish: intervals %.3f alleles %.3f ms; %lld entries, %lld intervals, %zu alleles kept\n", clk.ms[0], clk.ms[1], (long long)in.n, (long long)in.n_iv,
            out->w0.size());
}

}  // namespace mm
