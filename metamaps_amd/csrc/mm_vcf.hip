// The alleles of a run's alignments on the device (mm_vcf_events / _merge / _finish; mapDirectly --vcf; DESIGN.md section 1, "VCF"; the definition:
// mm_vcf_core.hpp, the text the host test runs).
//   events   mm_events.hpp's pipeline (count, scan, emit, sort, reduce) over two-word keys with VcfEvents:
//            count    vcf_count_kernel: one wavefront (a 64-thread workgroup) per job; the lanes stride over the runs, apply the rules and sum the job's bound of
//                     alleles (X bases + the I and D runs between other runs) and its indel runs, the second count: whether the call has an indel at all.
//                     A job that breaks a rule puts (job << 4 | rule) into the error word with an atomic minimum.
//            emit     vcf_emit_kernel: one wavefront per job over tiles of 64 runs; wave scans give each run its contig position, its read index and its
//                     place; a lane writes its own short run and left-aligns its own indel (a loop of at most NORM_MAX steps over EditSeq::byte on the
//                     job's contig, no shuffle inside), the wavefront expands an X run of more than 64 bases.  A skipped event is the all-ones pair.
//            sort     by w1, then by the bits of w0 in use.  A call without an indel sorts w0 alone: every w1 is 0 or all ones.  The all-ones pairs sort
//                     last and are cut off the table.
//   merge    mm_keytable.hip's merge_run over two-word keys.
//   finish   mm_keytable.hip's finish_kept with w1 and the reference window as a kept allele's payload.
// No kernel here waits for another workgroup; the only atomic is the error word's minimum.
// The jobs' arrays, their checks and the launch loop are mm_jobs_dev.hpp's, shared with every output that walks the jobs.
#include "mm_vcf.hpp"
#include "mm_events.hpp"
#include "mm_vcf_core.hpp"
#include "mm_prims.hpp"

namespace mm {

__global__ void __launch_bounds__(64) vcf_count_kernel(const int32_t* __restrict__ q_len, int64_t n_reads, const int32_t* __restrict__ r_len, int64_t n_contigs, AlignedJobs J,
                                                       const uint8_t* __restrict__ use, int64_t job0, int64_t* __restrict__ counts, int64_t* __restrict__ indels,
                                                       unsigned long long* __restrict__ err) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n) return;
  WaveLanes p;
  int64_t alleles = 0, ind = 0;
  int rule = 0;
  if (use[job] && J.dist[job] >= 0)
    rule = mmv::count_job(p, J.read[job], n_reads, J.contig[job], n_contigs, J.strand[job], q_len, r_len, J.first[job], J.ops + J.op_off[job], J.op_off[job + 1] - J.op_off[job], &alleles,
                          &ind);
  if (threadIdx.x == 0) {
    counts[job] = alleles; indels[job] = ind;
    if (rule) atomicMin(err, (unsigned long long)job << 4 | (unsigned long long)rule);
  }
}
// the alleles of job to w0 and w1 [off[job], off[job + 1]); a job without any (not used, not aligned, or nothing but = and edge runs) writes nothing
__global__ void __launch_bounds__(64) vcf_emit_kernel(EditSeq Q, const uint64_t* __restrict__ q_base, const int32_t* __restrict__ q_len, EditSeq R, const uint64_t* __restrict__ r_base,
                                                      AlignedJobs J, int64_t job0, const int64_t* __restrict__ off, const uint8_t* __restrict__ q_qual, int32_t qmin, uint64_t* __restrict__ w0,
                                                      uint64_t* __restrict__ w1) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n || off[job + 1] == off[job]) return;
  WaveLanes p;
  const int32_t read = J.read[job], contig = J.contig[job];
  const uint64_t qg = q_base[read];
  const int64_t m = q_len[read];
  mmv::emit_job_q(p, SeqBytes{Q.narrowed(qg, qg + (uint64_t)m), (int64_t)qg, q_qual}, m, J.strand[job], SeqBytes{R, (int64_t)r_base[contig]}, contig, J.first[job],
                  J.ops + J.op_off[job], J.op_off[job + 1] - J.op_off[job], qmin, w0 + off[job], w1 + off[job]);
}

struct VcfEvents {                                               // what mm_events.hpp's pipeline asks of a format
  static constexpr const char* who = "mm_vcf_events";
  static constexpr const char* timing = "MM_VCF_TIMING";
  static constexpr int32_t param_max = 93;
  static constexpr const char* param_text = "mm_vcf_events_q: min_base_quality is not in [0, 93]";
  static constexpr int64_t max_contigs = mmp::MAX_CONTIGS;
  static constexpr const char* contigs_text = "mm_vcf_events: more than 2^29 contigs";
  static constexpr int key_shift = mmp::CONTIG_SHIFT;
  static constexpr bool two_words = true;
  static constexpr const char* second = "indels";                 // without an indel every w1 is 0, or all ones beside an all-ones w0: w0 alone decides
  static constexpr uint64_t sentinel = mmv::SKIP;                  // the all-ones pair, the last segment where there is one, is no allele
  static bool cuts_sentinel(int32_t) { return true; }
  static int32_t value(const mm_seqset* reads, int32_t min_base_quality) { return reads->has_qual ? min_base_quality : 0; }   // (reads without qualities pass every floor)
  static const char* rule_text(int rule) { return mmv::rule_text(rule); }
  static void count(const EventsLaunch& L, int64_t a, dim3 grid) {
    vcf_count_kernel<<<grid, dim3(64), 0, L.st>>>(L.reads->d_len.p, L.reads->count(), L.ref->d_len.p, L.ref->count(), L.J, L.use, a, L.counts, L.counts2, L.err);
  }
  static void emit(const EventsLaunch& L, int64_t a, dim3 grid) {
    vcf_emit_kernel<<<grid, dim3(64), 0, L.st>>>(edit_seq(L.reads), L.reads->d_base.p, L.reads->d_len.p, edit_seq(L.ref), L.ref->d_base.p, L.J, a, L.off, L.reads->qual_ptr(), L.value, L.w0,
                                                 L.w1);
  }
};
void vcf_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const AlignedJobsIn& in, const uint8_t* use, int32_t min_base_quality, KeyTable* out) {
  key_events_run<VcfEvents>(ctx, reads, ref, in, use, min_base_quality, out);
}

struct VcfWindow {                                                // a kept allele's payload: its w1, and the reference's bytes from its position on (zero beyond the contig's end)
  EditSeq R; const uint64_t* r_base; const int32_t* r_len; const uint64_t* w1; uint64_t* o1; uint8_t* owin;
  __device__ void operator()(int64_t i, int64_t o, int64_t c, int64_t at) const {
    o1[o] = w1[i];
    const int64_t len = mmv::window_len(at, r_len[c]);
    for (int64_t t = 0; t < mmv::WINDOW; ++t) owin[o * mmv::WINDOW + t] = t < len ? R.byte((int64_t)r_base[c] + at + t) : (uint8_t)0;
  }
};

void vcf_finish_run(mm_ctx* ctx, const mm_seqset* ref, const FinishIn& in, VcfResult* out) {
  hipStream_t st = ctx->stream;
  StageClock<3> clk(getenv("MM_VCF_TIMING") != nullptr, st);       // intervals (upload and sorts), alleles
  const int64_t nc = ref->count();
  auto check_keys = [&] {                                         // before anything is launched: every later index is inside its array
    for (int64_t i = 0; i < in.n; ++i) {
      const uint64_t a = in.w0[i], b = in.w1[i];
      MM_REQUIRE(i == 0 || in.w0[i - 1] < a || (in.w0[i - 1] == a && in.w1[i - 1] < b), MM_ERR_ARG,
                 "mm_vcf_finish: the keys are not ascending and unique (entry " + std::to_string(i) + "): pass a merged table");
      MM_REQUIRE(mmp::key_contig(a) < nc && mmv::key_valid(a, b, ref->len[(size_t)mmp::key_contig(a)]), MM_ERR_ARG,
                 "mm_vcf_finish: entry " + std::to_string(i) + " names no position of the reference, or no allele");
    }
  };
  DBuf<uint64_t> d_w1, d_o1; DBuf<uint8_t> d_owin;
  auto compact = [&](const KeptDev& rows) {
    const size_t k = (size_t)rows.n;
    d_w1.alloc(k); d_o1.alloc(k); d_owin.alloc(k * mmv::WINDOW);
    d_w1.upload(in.w1, k, st);
    compact_kept(rows, VcfWindow{edit_seq(ref), ref->d_base.p, ref->d_len.p, d_w1.p, d_o1.p, d_owin.p}, st);
  };
  out->w1.clear(); out->window.clear();
  if (!finish_kept(ctx, ref, in, "mm_vcf_finish", check_keys, compact, clk, nullptr, out)) return;
  out->w1 = d_o1.to_host(st, out->w0.size()); out->window = d_owin.to_host(st, out->w0.size() * mmv::WINDOW);
  clk.stop(1);
  if (clk.on)
    fprintf(stderr, "MM_VCF_TIMING finish: intervals %.3f alleles %.3f ms; %lld entries, %lld intervals, %zu alleles kept\n", clk.ms[0], clk.ms[1], (long long)in.n, (long long)in.n_iv,
            out->w0.size());
}

}  // namespace mm
