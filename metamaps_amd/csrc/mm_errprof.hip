// The error profile of a run's alignments on the device (mm_errprof_events / _finish; mapDirectly --error-profile; DESIGN.md section 1, "Error profile"; the
// definition: mm_errprof_core.hpp, the text the host test runs).
//   events   check    errprof_check_kernel: one wavefront (a 64-thread workgroup) per job applies mmp::count_job's rules; a job that breaks one puts
//                     (job << 4 | rule) into the error word with an atomic minimum, and the host reads the word before anything else is launched.
//            walk     errprof_walk_kernel: G workgroups of one wavefront each, grid-stride over the jobs.  A job is walked over tiles of 64 runs: wave scans
//                     give each run its contig position and read index, a lane walks its own run of up to 64 bases, the wavefront a longer one.  The 566
//                     counters live in LDS as 32-bit words, added to with LDS atomics, and stay there across the workgroup's jobs.  Before a job that could
//                     carry a word past 2^32 - 1, and at its end, the workgroup adds its table to its own row of a G x 566 table of 64-bit partial sums:
//                     plain vector stores, no global atomic.  Lane 0 writes the job's six columns and its identity key.
//            sum      errprof_sum_kernel: one thread per counter adds the G rows.
//   finish   one sort_pairs of (key, index) over the bits in use and one sort of the ppm values alone; errprof_rows_kernel: one wavefront per contig finds its
//            segment by two binary searches, sums the six columns through the permutation and reads the five order statistics by rank; the row over all
//            alignments takes them from the second sort.
// No kernel here waits for another workgroup; the only global atomic is the error word's minimum.
#include "mm_errprof.hpp"
#include "mm_errprof_core.hpp"
#include "mm_keytable.hpp"
#include "mm_prims.hpp"
#include <string>

namespace mm {

constexpr int ERRPROF_GROUPS_PER_CU = 16;                         // the default G is this multiple of the device's CUs (profiles/errprof_stats.txt)
constexpr int64_t ERRPROF_GROUPS_MAX = 1 << 16;

// the walk's sink: the workgroup's table in LDS.  Plain LDS atomics measured faster than lane-private counts for the diagonal substitutions and the current
// quality row (walk 31.3 against 40.5 ms on the batch of profiles/errprof_stats.txt): the lanes of a wavefront walk different runs, and the branches cost more
// than the adds that meet on one word.
struct LdsCounters {
  uint32_t* tab;
  __device__ void add(uint32_t index) { atomicAdd(&tab[index], 1u); }
};

__global__ void __launch_bounds__(64) errprof_check_kernel(const int32_t* __restrict__ q_len, int64_t n_reads, const int32_t* __restrict__ r_len, int64_t n_contigs, AlignedJobs J,
                                                           const uint8_t* __restrict__ use, int64_t job0, unsigned long long* __restrict__ err) {
  const int64_t job = job0 + (int64_t)blockIdx.x;
  if (job >= J.n || !use[job] || J.dist[job] < 0) return;
  WaveLanes p;
  int64_t events = 0;
  const int rule = mmp::count_job(p, J.read[job], n_reads, J.contig[job], n_contigs, J.strand[job], q_len, r_len, J.first[job], J.ops + J.op_off[job], J.op_off[job + 1] - J.op_off[job], &events);
  if (threadIdx.x == 0 && rule) atomicMin(err, (unsigned long long)job << 4 | (unsigned long long)rule);
}

// the workgroup's table to its own row of the partial sums; the table starts again at zero
__device__ void errprof_flush(LdsCounters& t, unsigned long long* __restrict__ row) {
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < mmep::COUNTERS; k += 64) { row[k] += t.tab[k]; t.tab[k] = 0; }
  __syncthreads();
}
// jobs whose checks have passed; part[gridDim.x][COUNTERS] starts at zero
__global__ void __launch_bounds__(64) errprof_walk_kernel(EditSeq Q, const uint64_t* __restrict__ q_base, const int32_t* __restrict__ q_len, const uint8_t* __restrict__ q_qual, EditSeq R,
                                                          const uint64_t* __restrict__ r_base, const int32_t* __restrict__ r_len, AlignedJobs J, const uint8_t* __restrict__ use,
                                                          unsigned long long* __restrict__ part, int32_t* __restrict__ cols, uint64_t* __restrict__ keys) {
  __shared__ uint32_t tab[mmep::COUNTERS];
  for (uint32_t k = threadIdx.x; k < mmep::COUNTERS; k += 64) tab[k] = 0;
  __syncthreads();
  WaveLanes p;
  LdsCounters t{tab};
  unsigned long long* const row = part + (size_t)blockIdx.x * mmep::COUNTERS;
  uint64_t pending = 0;                                           // no word of the table has been added to more often since it was zero
  for (int64_t job = blockIdx.x; job < J.n; job += gridDim.x) {
    int64_t c[mmep::COLS] = {0, 0, 0, 0, 0, 0};
    uint64_t key = mmep::NO_KEY;
    if (use[job] && J.dist[job] >= 0) {
      const int32_t read = J.read[job], contig = J.contig[job];
      const uint64_t qg = q_base[read], rg = r_base[contig];
      const int64_t m = q_len[read], len = r_len[contig];
      const uint64_t most = (uint64_t)(m > len ? m : len);        // a job adds to one word once per read base or once per run of deleted bases at most
      if (pending + most > 0xFFFFFFFFull) { errprof_flush(t, row); pending = 0; }
      pending += most;
      mmep::walk_job(p, SeqBytes{Q.narrowed(qg, qg + (uint64_t)m), (int64_t)qg, q_qual}, SeqBytes{R.narrowed(rg, rg + (uint64_t)len), (int64_t)rg}, m, J.strand[job], J.first[job], len,
                     J.ops + J.op_off[job], J.op_off[job + 1] - J.op_off[job], t, c);
      key = mmep::ident_key(contig, c);
    }
    if (threadIdx.x == 0) {
      int32_t* const o = cols + job * mmep::COLS;
      o[0] = (int32_t)c[0]; o[1] = (int32_t)c[1]; o[2] = (int32_t)c[2]; o[3] = (int32_t)c[3]; o[4] = (int32_t)c[4]; o[5] = (int32_t)c[5];
      keys[job] = key;
    }
  }
  errprof_flush(t, row);
}
__global__ void __launch_bounds__(256) errprof_sum_kernel(const unsigned long long* __restrict__ part, int64_t groups, unsigned long long* __restrict__ counters) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= mmep::COUNTERS) return;
  unsigned long long s = 0;
  for (int64_t g = 0; g < groups; ++g) s += part[(size_t)g * mmep::COUNTERS + k];
  counters[k] = s;
}

static int64_t errprof_groups(const mm_ctx* ctx, int64_t n_jobs) {
  int64_t g = (int64_t)std::max(ctx->cus, 1) * ERRPROF_GROUPS_PER_CU;
  if (const char* e = getenv("MM_ERRPROF_GROUPS")) { const long long v = atoll(e); if (v >= 1) g = v; }
  return std::max<int64_t>(1, std::min({g, ERRPROF_GROUPS_MAX, n_jobs}));
}

void errprof_events_run(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* ref, const AlignedJobsIn& in, const uint8_t* use, uint64_t* counters, int32_t* cols, uint64_t* ident_key) {
  AlignedJobsDev jobs(ctx, reads, ref, in, "mm_errprof_events");
  MM_REQUIRE(ref->count() <= mmep::MAX_CONTIGS, MM_ERR_ARG, "mm_errprof_events: more than 2^31 contigs");
  std::fill(counters, counters + mmep::COUNTERS, (uint64_t)0);
  const int64_t n = in.n_jobs;
  if (n == 0) return;                                              // nothing is launched
  const size_t k = (size_t)n;
  hipStream_t st = ctx->stream;
  StageClock<4> clk(getenv("MM_ERRPROF_TIMING") != nullptr, st);   // upload, check, walk, sum (with the results' way to the host)

  clk.start();
  const AlignedJobs J = jobs.upload(st);
  const uint8_t* const d_use = jobs.upload_use(use, st);
  clk.stop(0);

  clk.start();
  for_job_grids(0, n, [&](int64_t a, dim3 grid) {
    errprof_check_kernel<<<grid, dim3(64), 0, st>>>(reads->d_len.p, reads->count(), ref->d_len.p, ref->count(), J, d_use, a, jobs.err.p);
  });
  jobs.require_no_error(st, mmp::rule_text);
  clk.stop(1);

  clk.start();
  const int64_t groups = errprof_groups(ctx, n);
  DBuf<unsigned long long> d_part((size_t)groups * mmep::COUNTERS), d_counters(mmep::COUNTERS);
  DBuf<int32_t> d_cols(k * mmep::COLS); DBuf<uint64_t> d_keys(k);
  d_part.zero(st);
  errprof_walk_kernel<<<dim3((unsigned)groups), dim3(64), 0, st>>>(edit_seq(reads), reads->d_base.p, reads->d_len.p, reads->qual_ptr(), edit_seq(ref), ref->d_base.p, ref->d_len.p, J, d_use,
                                                                   d_part.p, d_cols.p, d_keys.p); MM_KERNEL_CHECK();
  clk.stop(2);

  clk.start();
  errprof_sum_kernel<<<dim3((mmep::COUNTERS + 255) / 256), dim3(256), 0, st>>>(d_part.p, groups, d_counters.p); MM_KERNEL_CHECK();
  d_cols.download(cols, k * mmep::COLS, st); d_keys.download(ident_key, k, st);
  const std::vector<unsigned long long> sums = d_counters.to_host(st);
  std::copy(sums.begin(), sums.end(), counters);
  clk.stop(3);
  if (clk.on)
    fprintf(stderr, "MM_ERRPROF_TIMING events: upload %.3f check %.3f walk %.3f sum %.3f ms; %lld jobs, %lld runs, %lld groups\n", clk.ms[0], clk.ms[1], clk.ms[2], clk.ms[3], (long long)n,
            (long long)jobs.n_ops, (long long)groups);
}

__global__ void __launch_bounds__(256) errprof_ppm_kernel(const uint64_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ ppm, uint32_t* __restrict__ index) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { ppm[i] = (uint32_t)mmep::key_ppm(keys[i]); index[i] = (uint32_t)i; }
}
// stats[(n_contigs + 1) * STATS]: row c of contig c from its segment of the sorted keys, row n_contigs over all n entries (its ranks from sppm, the ppm
// values sorted alone); a contig without entries gets zeros
__global__ void __launch_bounds__(64) errprof_rows_kernel(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ sppm,
                                                          const int32_t* __restrict__ cols, int64_t n, int64_t n_contigs, int64_t* __restrict__ stats) {
  for (int64_t row = blockIdx.x; row <= n_contigs; row += gridDim.x) {
    const bool all = row == n_contigs;
    const int64_t lo = all ? 0 : mmp::bound(skey, n, (uint64_t)row << 32, false), hi = all ? n : mmp::bound(skey, n, (uint64_t)(row + 1) << 32, false);
    long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
    for (int64_t a = lo + threadIdx.x; a < hi; a += 64) {
      const int32_t* const c = cols + (int64_t)perm[a] * mmep::COLS;
      s0 += c[0]; s1 += c[1]; s2 += c[2]; s3 += c[3]; s4 += c[4]; s5 += c[5];
    }
    for (int d = 32; d > 0; d >>= 1) {
      s0 += __shfl_xor(s0, d, 64); s1 += __shfl_xor(s1, d, 64); s2 += __shfl_xor(s2, d, 64); s3 += __shfl_xor(s3, d, 64); s4 += __shfl_xor(s4, d, 64); s5 += __shfl_xor(s5, d, 64);
    }
    int64_t* const o = stats + row * mmep::STATS;
    const int64_t cnt = hi - lo;
    if (threadIdx.x == 0) { o[mmep::ALIGNMENTS] = cnt; o[1] = s0; o[2] = s1; o[3] = s2; o[4] = s3; o[5] = s4; o[6] = s5; }
    if (threadIdx.x >= mmep::PPM_MIN && threadIdx.x <= mmep::PPM_MAX) {
      const int64_t at = cnt > 0 ? lo + mmep::rank_of((int)threadIdx.x, cnt) : 0;
      o[threadIdx.x] = cnt <= 0 ? 0 : all ? (int64_t)sppm[at] : mmep::key_ppm(skey[at]);
    }
  }
}

void errprof_finish_run(mm_ctx* ctx, int64_t n_contigs, int64_t n, const uint64_t* ident_key, const int32_t* cols, ErrprofResult* out) {
  const std::string who = "mm_errprof_finish: ";
  MM_REQUIRE(n_contigs >= 0 && n_contigs <= mmep::MAX_CONTIGS, MM_ERR_ARG, who + "a negative number of contigs, or more than 2^31");
  std::vector<uint64_t> keys; std::vector<int32_t> kept;           // before anything is launched: the entries that count, every contig inside the rows
  for (int64_t i = 0; i < n; ++i) {
    if (ident_key[i] == mmep::NO_KEY) continue;
    MM_REQUIRE(mmep::key_contig(ident_key[i]) < n_contigs, MM_ERR_ARG, who + "entry " + std::to_string(i) + " names contig " + std::to_string(mmep::key_contig(ident_key[i])) + " of " +
               std::to_string(n_contigs));
    keys.push_back(ident_key[i]);
    kept.insert(kept.end(), cols + i * mmep::COLS, cols + (i + 1) * mmep::COLS);
  }
  out->contig.clear();
  out->stats.assign(mmep::STATS, 0);                               // (the row over all alignments alone)
  const size_t v = keys.size(), rows = (size_t)n_contigs + 1;
  if (v == 0) return;                                              // nothing is launched
  MM_REQUIRE(v < ((size_t)1 << 32), MM_ERR_LIMIT, who + "2^32 entries or more");

  hipStream_t st = ctx->stream;
  StageClock<2> clk(getenv("MM_ERRPROF_TIMING") != nullptr, st);   // sort (with the upload), rows (with their way to the host)
  clk.start();
  DBuf<uint64_t> d_keys(v), d_skey(v); DBuf<uint32_t> d_index(v), d_perm(v), d_ppm(v), d_sppm(v); DBuf<int32_t> d_cols(v * mmep::COLS); DBuf<uint8_t> tmp;
  d_keys.upload(keys.data(), v, st); d_cols.upload(kept.data(), v * mmep::COLS, st);
  errprof_ppm_kernel<<<dim3(flat_grid((int64_t)v)), dim3(256), 0, st>>>(d_keys.p, (int64_t)v, d_ppm.p, d_index.p); MM_KERNEL_CHECK();
  sort_pairs(tmp, d_keys.p, d_skey.p, d_index.p, d_perm.p, v, 0, 32 + contig_bits(n_contigs), st);
  sort_keys(tmp, d_ppm.p, d_sppm.p, v, 0, 20, st);                 // (ppm <= 10^6 < 2^20)
  clk.stop(0);

  clk.start();
  DBuf<int64_t> d_stats(rows * mmep::STATS);
  errprof_rows_kernel<<<dim3((unsigned)std::min<size_t>(rows, 65536)), dim3(64), 0, st>>>(d_skey.p, d_perm.p, d_sppm.p, d_cols.p, (int64_t)v, n_contigs, d_stats.p); MM_KERNEL_CHECK();
  const std::vector<int64_t> stats = d_stats.to_host(st);
  clk.stop(1);
  out->stats.clear();
  for (int64_t c = 0; c < n_contigs; ++c)
    if (stats[(size_t)c * mmep::STATS + mmep::ALIGNMENTS] > 0) {
      out->contig.push_back((int32_t)c);
      out->stats.insert(out->stats.end(), stats.begin() + c * mmep::STATS, stats.begin() + (c + 1) * mmep::STATS);
    }
  out->stats.insert(out->stats.end(), stats.begin() + n_contigs * mmep::STATS, stats.end());
  if (clk.on) fprintf(stderr, "MM_ERRPROF_TIMING finish: sort %.3f rows %.3f ms; %zu entries, %zu contigs listed\n", clk.ms[0], clk.ms[1], v, out->contig.size());
}

}  // namespace mm
