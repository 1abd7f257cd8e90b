// The events of a batch's aligned jobs as a key table, once for every format that emits keys per job (mm_pileup.hip, mm_vcf.hip, mm_mods.hip; DESIGN.md
// section 1, "Aligned jobs and key tables").  key_events_run<F> is the pipeline; a format F is a struct of constants and two launches:
//   who, timing          the entry point's name, which the messages start with, and the variable that asks for the stage times (and starts their line)
//   param_max, param_text, max_contigs, contigs_text
//                        the call's one parameter lies in [0, param_max] and the reference has max_contigs contigs at most, or MM_ERR_ARG with that text
//   value(reads, param)  what the kernels get for the parameter
//   rule_text(rule)      the text of a rule that the count kernel found broken
//   key_shift            the bits of w0 below the contig: the sort goes over key_shift + the contig's bits
//   two_words            rows are (w0, w1) pairs, sorted by w1 and then by w0, 20 bytes a row in the table; else w0 alone and 12 bytes
//   second               null, or with two-word keys the name in the timing line of their second per-job count: the rows whose w1 decides their order; where
//                        a call has none, w0 alone is sorted and the table's w1 is zeros
//   sentinel, cuts_sentinel(value)
//                        the key that the emit kernel leaves in the place of a row that is none; it sorts last, and its segment is cut where cuts_sentinel
//   count(L, job0, grid), emit(L, job0, grid)
//                        launch the format's count kernel (into L.counts, L.counts2 and L.err) and its emit kernel (rows of job j to L.w0, L.w1 from
//                        L.off[j] on) for the jobs from job0 on, one wavefront per job
#pragma once
#include "mm_jobs_dev.hpp"
#include "mm_keytable.hpp"
#include <cstdio>
#include <string>

namespace mm {

struct EventsLaunch {                                             // what a format's two launches read; counts2 and w1 are null where the format has none
  const mm_seqset* reads; const mm_seqset* ref; AlignedJobs J; const uint8_t* use; int32_t value; hipStream_t st;
  int64_t* counts; int64_t* counts2; unsigned long long* err;
  const int64_t* off; uint64_t* w0; uint64_t* w1;
};

// Stage by stage: upload (the jobs, `use`, zeroed counts), count (the host reads the error word before anything else is launched), scan (with the one wait
// of the call: the totals), emit, sort, reduce (with the table's way to the host).  No job, or no event: nothing further is allocated or launched.
template <class F> void key_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const AlignedJobsIn& in, const uint8_t* use, int32_t param, KeyTable* out) {
  constexpr bool has_second = F::second != nullptr;
  static_assert(F::two_words == has_second, "two-word keys come with the count of the rows whose w1 decides their order");
  AlignedJobsDev jobs(ctx, reads, ref, in, F::who);
  MM_REQUIRE(param >= 0 && param <= F::param_max, MM_ERR_ARG, F::param_text);
  MM_REQUIRE(ref->count() <= F::max_contigs, MM_ERR_ARG, F::contigs_text);
  out->clear();
  const int64_t n = in.n_jobs;
  if (n == 0) return;
  const size_t k = (size_t)n;
  hipStream_t st = ctx->stream;
  StageClock<6> clk(getenv(F::timing) != nullptr, st);

  clk.start();
  EventsLaunch L{reads, ref, jobs.upload(st), nullptr, F::value(reads, param), st, nullptr, nullptr, jobs.err.p, nullptr, nullptr, nullptr};
  DBuf<int64_t> d_counts(k + 1), d_off(k + 1), d_counts2, d_off2;
  L.use = jobs.upload_use(use, st);
  d_counts.zero(st);
  if (has_second) { d_counts2.alloc(k + 1); d_off2.alloc(k + 1); d_counts2.zero(st); }
  L.counts = d_counts.p; L.counts2 = d_counts2.p; L.off = d_off.p;
  clk.stop(0);

  clk.start();
  for_job_grids(0, n, [&](int64_t a, dim3 grid) { F::count(L, a, grid); });
  jobs.require_no_error(st, F::rule_text);
  clk.stop(1);

  clk.start();
  DBuf<uint8_t> tmp;
  int64_t total = 0, second = 0;
  exclusive_scan(tmp, d_counts.p, d_off.p, k + 1, st);
  if (has_second) exclusive_scan(tmp, d_counts2.p, d_off2.p, k + 1, st);
  d_off.download(&total, 1, st, k);
  if (has_second) d_off2.download(&second, 1, st, k);
  MM_HIP(mm::stream_sync(st));
  clk.stop(2);
  MM_REQUIRE(total < ((int64_t)1 << 32), MM_ERR_LIMIT, std::string(F::who) + ": 2^32 events or more in one call");
  if (total > 0) {
    const bool by_w1 = second > 0;
    clk.start();
    DBuf<uint64_t> d_w0((size_t)total), d_w1(F::two_words ? (size_t)total : 0);
    L.w0 = d_w0.p; L.w1 = d_w1.p;
    for_job_grids(0, n, [&](int64_t a, dim3 grid) { F::emit(L, a, grid); });
    clk.stop(3);
    clk.start();
    SortedTable sorted;
    sort_table(tmp, d_w0.p, by_w1 ? d_w1.p : nullptr, nullptr, total, F::key_shift + contig_bits(ref->count()), F::two_words ? 64 : 0, st, &sorted);
    if (by_w1) { MM_HIP(mm::stream_sync(st)); sorted.perm.release(); sorted.i1.release(); }   // (the two index buffers go once the sort is through: the reduction takes their blocks)
    clk.stop(4);
    clk.start();
    reduce_sorted(tmp, sorted, total, st, out);
    if (F::two_words && !by_w1) out->w1.assign(out->w0.size(), 0);
    if (F::cuts_sentinel(L.value) && !out->w0.empty() && out->w0.back() == F::sentinel) {   // the rows that are none: the last segment
      out->w0.pop_back(); out->counts.pop_back();
      if (F::two_words) out->w1.pop_back();
    }
    clk.stop(5);
  }
  if (clk.on) {
    std::string of_second;
    if constexpr (has_second) of_second = " (" + std::to_string(second) + " " + F::second + ")";
    fprintf(stderr, "%s events: upload %.3f count %.3f scan %.3f emit %.3f sort %.3f reduce %.3f ms; %lld jobs, %lld runs, %lld events%s, %zu pairs, %zu B fetched\n", F::timing, clk.ms[0],
            clk.ms[1], clk.ms[2], clk.ms[3], clk.ms[4], clk.ms[5], (long long)n, (long long)jobs.n_ops, (long long)total, of_second.c_str(), out->w0.size(),
            out->w0.size() * (F::two_words ? 20 : 12));
  }
}

}  // namespace mm
