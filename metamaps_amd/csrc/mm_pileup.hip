// The pileup of a run's alignments on the device (mm_pileup_events / _merge / _finish; mapDirectly --pileup; DESIGN.md section 1, "Pileup"; the
// definition: mm_pileup_core.hpp, the text the host test runs).
//   events   count    pile_count_kernel: one wavefront (a 64-thread workgroup) per job; the lanes stride over the runs, sum the job's events and apply the
//                     rules.  A job that breaks one puts (job << 4 | rule) into the error word with an atomic minimum; the host reads the word before
//                     anything else is launched.
//            scan     an exclusive scan of the counts (mm_prims.hpp) places every job's events.
//            emit     pile_emit_kernel: one wavefront per job over tiles of 64 runs; a wave scan of the run lengths gives each run its contig position,
//                     its read index and its place; a lane expands its own short run, the wavefront a run of more than 64 events.  Read bases come
//                     through EditSeq::byte on a set narrowed to the read.  Keys are stored as 8-byte words, nothing else is written.
//            reduce   one radix sort of the keys over the bits in use, then the segments of equal keys with their lengths (mm_keytable.hip).
//            floor    mm_pileup_events_q: the emit kernel reads the reads' quality plane beside the bases and writes mmp::DROPPED in the place of an event
//                     under the floor; every bit of it in use is set, so it sorts last, and its segment is cut off the table.  Floor 0: nothing differs.
//   merge    mm_keytable.hip's merge_run over one-word keys: sort_pairs of (key, count) and the sums of the segments.
//   finish   mm_keytable.hip's finish_kept with the reference's byte as a kept site's payload; per contig the alignments, the summed lengths and the
//            union's length (each interval adds what lies beyond the running maximum of the ends before it, an inclusive max-scan) with 64-bit vector atomics.
// No kernel here waits for another workgroup; the only atomics are the error word's minimum and the per-contig sums.
// The jobs' arrays, their checks and the launch loop are mm_jobs_dev.hpp's, shared with mm_bam.hip and mm_vcf.hip.
#include "mm_pileup.hpp"
#include "mm_pileup_core.hpp"
#include "mm_prims.hpp"

namespace mm {

__global__ void __launch_bounds__(64) pile_count_kernel(const int32_t* __restrict__ q_len, int64_t n_reads, const int32_t* __restrict__ r_len, int64_t n_contigs, AlignedJobs J,
                                                        const uint8_t* __restrict__ use, int64_t job0, int64_t* __restrict__ counts, unsigned long long* __restrict__ err) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n) return;
  WaveLanes p;
  int64_t events = 0;
  int rule = 0;
  if (use[job] && J.dist[job] >= 0)
    rule = mmp::count_job(p, J.read[job], n_reads, J.contig[job], n_contigs, J.strand[job], q_len, r_len, J.first[job], J.ops + J.op_off[job], J.op_off[job + 1] - J.op_off[job], &events);
  if (threadIdx.x == 0) {
    counts[job] = events;
    if (rule) atomicMin(err, (unsigned long long)job << 4 | (unsigned long long)rule);
  }
}
// the events of job to keys[off[job], off[job + 1]); a job without events (not used, not aligned, or all =) writes nothing
__global__ void __launch_bounds__(64) pile_emit_kernel(EditSeq Q, const uint64_t* __restrict__ q_base, const int32_t* __restrict__ q_len, AlignedJobs J, int64_t job0,
                                                       const int64_t* __restrict__ off, const uint8_t* __restrict__ q_qual, int32_t qmin, uint64_t* __restrict__ keys) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n || off[job + 1] == off[job]) return;
  WaveLanes p;
  const int32_t read = J.read[job];
  const uint64_t qg = q_base[read];
  const int64_t m = q_len[read];
  mmp::emit_job_q(p, SeqBytes{Q.narrowed(qg, qg + (uint64_t)m), (int64_t)qg, q_qual}, m, J.strand[job], J.contig[job], J.first[job], J.ops + J.op_off[job],
                  J.op_off[job + 1] - J.op_off[job], qmin, keys + off[job]);
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

void pileup_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const AlignedJobsIn& in, const uint8_t* use, int32_t min_base_quality, KeyTable* out) {
  AlignedJobsDev jobs(ctx, reads, ref, in, "mm_pileup_events");
  MM_REQUIRE(min_base_quality >= 0 && min_base_quality <= 93, MM_ERR_ARG, "mm_pileup_events_q: min_base_quality is not in [0, 93]");
  const int32_t qmin = reads->has_qual ? min_base_quality : 0;     // (reads without qualities pass every floor)
  MM_REQUIRE(ref->count() <= mmp::MAX_CONTIGS, MM_ERR_ARG, "mm_pileup_events: more than 2^29 contigs");
  out->clear();
  const int64_t n = in.n_jobs;
  if (n == 0) return;
  const size_t k = (size_t)n;
  hipStream_t st = ctx->stream;
  StageClock<6> clk(getenv("MM_PILEUP_TIMING") != nullptr, st);    // upload, count, scan, emit, sort, reduce (with the table's way to the host)

  clk.start();
  const AlignedJobs J = jobs.upload(st);
  DBuf<int64_t> d_counts(k + 1), d_off(k + 1);
  DBuf<uint8_t> d_use(k);
  d_use.upload(use, k, st);
  d_counts.zero(st);
  clk.stop(0);

  clk.start();
  for_job_grids(0, n, [&](int64_t a, dim3 grid) {
    pile_count_kernel<<<grid, dim3(64), 0, st>>>(reads->d_len.p, reads->count(), ref->d_len.p, ref->count(), J, d_use.p, a, d_counts.p, jobs.err.p);
  });
  jobs.require_no_error(st, mmp::rule_text);
  clk.stop(1);

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
    DBuf<uint64_t> d_keys((size_t)total);
    for_job_grids(0, n, [&](int64_t a, dim3 grid) {
      pile_emit_kernel<<<grid, dim3(64), 0, st>>>(edit_seq(reads), reads->d_base.p, reads->d_len.p, J, a, d_off.p, reads->qual_ptr(), qmin, d_keys.p);
    });
    clk.stop(3);
    clk.start();
    SortedTable sorted;
    sort_table(tmp, d_keys.p, nullptr, nullptr, total, mmp::CONTIG_SHIFT + contig_bits(ref->count()), 0, st, &sorted);
    clk.stop(4);
    clk.start();
    reduce_sorted(tmp, sorted, total, st, out);
    if (qmin > 0 && !out->w0.empty() && out->w0.back() == mmp::DROPPED) { out->w0.pop_back(); out->counts.pop_back(); }   // the events under the floor: the last segment
    clk.stop(5);
  }
  if (clk.on)
    fprintf(stderr, "MM_PILEUP_TIMING events: upload %.3f count %.3f scan %.3f emit %.3f sort %.3f reduce %.3f ms; %lld jobs, %lld runs, %lld events, %zu pairs, %zu B fetched\n", clk.ms[0],
            clk.ms[1], clk.ms[2], clk.ms[3], clk.ms[4], clk.ms[5], (long long)n, (long long)jobs.n_ops, (long long)total, out->w0.size(), out->w0.size() * 12);
}

struct PileRefByte {                                              // a kept site's payload: the reference's byte at its position
  EditSeq R; const uint64_t* r_base; uint8_t* oref;
  __device__ void operator()(int64_t, int64_t o, int64_t contig, int64_t at) const { oref[o] = R.byte((int64_t)r_base[contig] + at); }
};

void pileup_finish_run(mm_ctx* ctx, const mm_seqset* ref, const FinishIn& in, PileupResult* out) {
  hipStream_t st = ctx->stream;
  StageClock<3> clk(getenv("MM_PILEUP_TIMING") != nullptr, st);    // intervals (upload and sorts), sites, coverage
  const int64_t n_contigs = ref->count();
  auto check_keys = [&] {                                         // before anything is launched: every later index is inside its array
    for (int64_t i = 0; i < in.n; ++i) {
      const uint64_t key = in.w0[i];
      MM_REQUIRE(i == 0 || in.w0[i - 1] < key, MM_ERR_ARG, "mm_pileup_finish: the keys are not ascending and unique (entry " + std::to_string(i) + "): pass a merged table");
      MM_REQUIRE(mmp::key_contig(key) < n_contigs && mmp::key_pos(key) < ref->len[(size_t)mmp::key_contig(key)] && mmp::key_code(key) < mmp::N_CODES, MM_ERR_ARG,
                 "mm_pileup_finish: entry " + std::to_string(i) + " names no position of the reference, or no code");
    }
  };
  DBuf<uint8_t> d_oref;
  auto compact = [&](const KeptDev& rows) { d_oref.alloc((size_t)rows.n); compact_kept(rows, PileRefByte{edit_seq(ref), ref->d_base.p, d_oref.p}, st); };
  SortedIntervals iv;
  const size_t nc = (size_t)n_contigs, v = (size_t)in.n_iv;
  out->ref_byte.clear();
  out->alignments.assign(nc, 0); out->covered.assign(nc, 0); out->sum_depth.assign(nc, 0);
  if (!finish_kept(ctx, ref, in, "mm_pileup_finish", check_keys, compact, clk, &iv, out)) return;
  out->ref_byte = d_oref.to_host(st, out->w0.size());
  clk.stop(1);

  clk.start();
  if (v) {
    DBuf<uint64_t> d_pmax(v); DBuf<unsigned long long> d_sums(3 * nc); DBuf<uint8_t> tmp;
    d_sums.zero(st);
    with_scratch(tmp, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, iv.end_of.p, d_pmax.p, v, rocprim::maximum<uint64_t>(), st); });
    pile_coverage_kernel<<<dim3(flat_grid(in.n_iv)), dim3(256), 0, st>>>(iv.starts.p, iv.end_of.p, d_pmax.p, in.n_iv, d_sums.p, d_sums.p + nc, d_sums.p + 2 * nc); MM_KERNEL_CHECK();
    const std::vector<unsigned long long> s = d_sums.to_host(st);
    for (size_t c = 0; c < nc; ++c) { out->alignments[c] = (int64_t)s[c]; out->covered[c] = (int64_t)s[nc + c]; out->sum_depth[c] = (int64_t)s[2 * nc + c]; }
  }
  clk.stop(2);
  if (clk.on)
    fprintf(stderr, "MM_PILEUP_TIMING finish: intervals %.3f sites %.3f coverage %.3f ms; %lld entries, %lld intervals, %zu sites kept\n", clk.ms[0], clk.ms[1], clk.ms[2], (long long)in.n,
            (long long)in.n_iv, out->w0.size());
}

}  // namespace mm
