// The pileup of a run's alignments on the device (mm_pileup_events / _merge / _finish; mapDirectly --pileup; DESIGN.md section 1, "Pileup"; the
// definition: mm_pileup_core.hpp, the text the host test runs).
//   events   mm_events.hpp's pipeline (count, scan, emit, sort, reduce) over one-word keys with PileupEvents:
//            count    pile_count_kernel: one wavefront (a 64-thread workgroup) per job; the lanes stride over the runs, sum the job's events and apply the
//                     rules.  A job that breaks one puts (job << 4 | rule) into the error word with an atomic minimum.
//            emit     pile_emit_kernel: one wavefront per job over tiles of 64 runs; a wave scan of the run lengths gives each run its contig position,
//                     its read index and its place; a lane expands its own short run, the wavefront a run of more than 64 events.  Read bases come
//                     through EditSeq::byte on a set narrowed to the read.  Keys are stored as 8-byte words, nothing else is written.
//            floor    mm_pileup_events_q: the emit kernel reads the reads' quality plane beside the bases and writes mmp::DROPPED in the place of an event
//                     under the floor; its segment, the last, is cut off the table.  Floor 0: nothing differs.
//   merge    mm_keytable.hip's merge_run over one-word keys: sort_pairs of (key, count) and the sums of the segments.
//   finish   mm_keytable.hip's finish_kept with the reference's byte as a kept site's payload; per contig the alignments, the summed lengths and the
//            union's length (each interval adds what lies beyond the running maximum of the ends before it, an inclusive max-scan) with 64-bit vector atomics.
// No kernel here waits for another workgroup; the only atomics are the error word's minimum and the per-contig sums.
// The jobs' arrays, their checks and the launch loop are mm_jobs_dev.hpp's, shared with every output that walks the jobs.
#include "mm_pileup.hpp"
#include "mm_events.hpp"
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

struct PileupEvents {                                            // what mm_events.hpp's pipeline asks of a format
  static constexpr const char* who = "mm_pileup_events";
  static constexpr const char* timing = "MM_PILEUP_TIMING";
  static constexpr int32_t param_max = 93;
  static constexpr const char* param_text = "mm_pileup_events_q: min_base_quality is not in [0, 93]";
  static constexpr int64_t max_contigs = mmp::MAX_CONTIGS;
  static constexpr const char* contigs_text = "mm_pileup_events: more than 2^29 contigs";
  static constexpr int key_shift = mmp::CONTIG_SHIFT;
  static constexpr bool two_words = false;
  static constexpr const char* second = nullptr;
  static constexpr uint64_t sentinel = mmp::DROPPED;               // an event under the floor; every bit of it in use is set, so it sorts last
  static bool cuts_sentinel(int32_t qmin) { return qmin > 0; }
  static int32_t value(const mm_seqset* reads, int32_t min_base_quality) { return reads->has_qual ? min_base_quality : 0; }   // (reads without qualities pass every floor)
  static const char* rule_text(int rule) { return mmp::rule_text(rule); }
  static void count(const EventsLaunch& L, int64_t a, dim3 grid) {
    pile_count_kernel<<<grid, dim3(64), 0, L.st>>>(L.reads->d_len.p, L.reads->count(), L.ref->d_len.p, L.ref->count(), L.J, L.use, a, L.counts, L.err);
  }
  static void emit(const EventsLaunch& L, int64_t a, dim3 grid) {
    pile_emit_kernel<<<grid, dim3(64), 0, L.st>>>(edit_seq(L.reads), L.reads->d_base.p, L.reads->d_len.p, L.J, a, L.off, L.reads->qual_ptr(), L.value, L.w0);
  }
};
void pileup_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const AlignedJobsIn& in, const uint8_t* use, int32_t min_base_quality, KeyTable* out) {
  key_events_run<PileupEvents>(ctx, reads, ref, in, use, min_base_quality, out);
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
