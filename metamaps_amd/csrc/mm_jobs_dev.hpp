// A batch's aligned jobs on the device, once for every output that walks them (mm_bam.hip, mm_pileup.hip, mm_vcf.hip, mm_mods.hip, mm_errprof.hip; DESIGN.md
// section 1, "Aligned jobs"): the lane policy of their one-wavefront-per-job kernels, the byte view of a sequence, the jobs' common arrays with their checks and
// uploads, the launch loop and the error word.  `use`, one byte per job that every output but BAM reads, is an optional column of AlignedJobsDev and a plain
// pointer beside AlignedJobs in a kernel's arguments; the columns that BAM alone reads (flag, mapq and the names) stay with it, in a struct of its own.
#pragma once
#include "mm_common.hpp"
#include "mm_edit_seq.hpp"
#include <algorithm>
#include <string>

namespace mm {

struct WaveLanes {                                                // one lane per thread of a 64-thread workgroup
  static constexpr uint32_t W = 64;
  __device__ uint32_t lane() const { return threadIdx.x; }
  __device__ int64_t scan_add(int64_t v, int64_t* total) const {
    long long x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long y = __shfl_up(x, o, 64); if ((int)threadIdx.x >= o) x += y; }
    *total = (int64_t)__shfl(x, 63, 64);
    return (int64_t)x - v;
  }
  __device__ int64_t scan_max(int64_t v, int64_t* total) const {  // of values >= 0; the lowest lane gets 0
    long long x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long y = __shfl_up(x, o, 64); if ((int)threadIdx.x >= o && y > x) x = y; }
    *total = (int64_t)__shfl(x, 63, 64);
    const long long below = __shfl_up(x, 1, 64);
    return threadIdx.x ? (int64_t)below : 0;
  }
  __device__ uint64_t ballot(bool b) const { return (uint64_t)__ballot(b); }
  __device__ int64_t pick(int64_t v, uint32_t l) const { return (int64_t)__shfl((long long)v, (int)l, 64); }
};
struct SeqBytes {                                                 // read (or contig) coordinate -> the set's byte, and the byte of its quality plane (null: no plane)
  EditSeq s; int64_t g0; const uint8_t* q = nullptr;
  __device__ uint8_t byte(int64_t i) const { return s.byte(g0 + i); }
  __device__ uint8_t qual(int64_t i) const { return q ? q[g0 + i] : (uint8_t)0xFF; }
};

constexpr unsigned long long JOB_NO_ERROR = ~0ull;
constexpr int64_t JOB_GRID_MAX = (int64_t)1 << 30;                // workgroups per launch

// the caller's arrays, as mm_bam_encode and the *_events entry points take them
struct AlignedJobsIn {
  int64_t n_jobs; const int32_t* read; const int32_t* strand; const int32_t* contig; const int32_t* dist; const int64_t* first;
  const int64_t* op_off; const uint32_t* ops;
};
// the same arrays on the device, as the kernels take them by value
struct AlignedJobs {
  int64_t n; const int32_t* read; const int32_t* strand; const int32_t* contig; const int32_t* dist; const int64_t* first;
  const int64_t* op_off; const uint32_t* ops;
};

// `off` starts at 0 or more and never falls (MM_ERR_ARG in the name of `who`); what: the array's name
inline void offsets_check(const int64_t* off, int64_t n, const char* who, const char* what) {
  bool ok = off[0] >= 0;
  for (int64_t i = 0; ok && i < n; ++i) ok = off[i] <= off[i + 1];
  MM_REQUIRE(ok, MM_ERR_ARG, std::string(who) + ": " + what + " does not start at 0 or more, or falls");
}

// fn(first job, workgroups) launches a one-wavefront-per-job kernel over the jobs [job0, job1), in pieces that a grid holds
template <class Launch> void for_job_grids(int64_t job0, int64_t job1, Launch&& fn) {
  for (int64_t a = job0; a < job1; a += JOB_GRID_MAX) { fn(a, dim3((unsigned)std::min(JOB_GRID_MAX, job1 - a))); MM_KERNEL_CHECK(); }
}

// The owner of a call's jobs on the device.  who: the entry point's name, which every message starts with.
struct AlignedJobsDev {
  const AlignedJobsIn in; const char* const who; size_t n_ops = 0;
  DBuf<int32_t> read, strand, contig, dist; DBuf<int64_t> first, op_off; DBuf<uint32_t> ops; DBuf<uint8_t> use;
  DBuf<unsigned long long> err;                                  // the kernels' error word: the smallest (job << 4 | rule) of the jobs that break a rule

  // what is asked of the sets and of the arrays before anything is launched
  AlignedJobsDev(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const AlignedJobsIn& in_, const char* who_) : in(in_), who(who_) {
    MM_REQUIRE(reads->frozen && ref->frozen, MM_ERR_STATE, std::string(who) + ": a sequence set is not uploaded");
    MM_REQUIRE(reads->ctx->device == ctx->device && ref->ctx->device == ctx->device, MM_ERR_ARG, std::string(who) + ": a sequence set lives on another device");
    if (in.n_jobs == 0) return;
    offsets_check(in.op_off, in.n_jobs, who, "op_off");
    n_ops = (size_t)in.op_off[in.n_jobs];
    MM_REQUIRE(n_ops == 0 || in.ops, MM_ERR_ARG, std::string(who) + ": a null array");
  }
  AlignedJobs upload(hipStream_t st) {                            // n_jobs > 0; the error word is set to "no job"
    const size_t k = (size_t)in.n_jobs;
    read.alloc(k); strand.alloc(k); contig.alloc(k); dist.alloc(k); first.alloc(k); op_off.alloc(k + 1); ops.alloc(std::max<size_t>(n_ops, 1)); err.alloc(1);
    read.upload(in.read, k, st); strand.upload(in.strand, k, st); contig.upload(in.contig, k, st); dist.upload(in.dist, k, st); first.upload(in.first, k, st);
    op_off.upload(in.op_off, k + 1, st); ops.upload(in.ops, n_ops, st);
    MM_HIP(hipMemsetAsync(err.p, 0xFF, sizeof(unsigned long long), st));
    return AlignedJobs{in.n_jobs, read.p, strand.p, contig.p, dist.p, first.p, op_off.p, ops.p};
  }
  const uint8_t* upload_use(const uint8_t* u, hipStream_t st) {   // n_jobs > 0; the optional column, one byte per job: its place on the device
    use.alloc((size_t)in.n_jobs);
    use.upload(u, (size_t)in.n_jobs, st);
    return use.p;
  }
  // The host reads the error word before anything else is launched: the kernels behind the first one trust what it checked.
  void require_no_error(hipStream_t st, const char* (*rule_text)(int)) const {
    const unsigned long long e = err.to_host(st)[0];
    MM_REQUIRE(e == JOB_NO_ERROR, MM_ERR_ARG, std::string(who) + ": job " + std::to_string(e >> 4) + ": " + rule_text((int)(e & 15)));
  }
};

}  // namespace mm
