// The depth profile of a run's alignments on the device (mm_depth_profile; mapDirectly --depth; DESIGN.md section 1, "Depth"; the definition:
// mm_depth_core.hpp, the text the host test runs).  Depth changes only at the 2 n_iv interval ends, so no array here is indexed by a reference position:
// device memory is O(n_iv + listed contigs + windows), and a contig of 2^29 - 1 bases costs what a contig of 100 does.
//   intervals    mm_keytable.hip's sorted_interval_keys: the keys of every first base and of every last base, each sorted.
//   breakpoints  depth_breaks_kernel: the 2 n_iv keys contig << 32 | first and contig << 32 | last + 1; one radix sort; head flags, a scan and a scatter leave
//                them unique; depth_piece_kernel: the depth behind each from two binary searches (mmp::depth_at's form).
//   runs         depth_runhead_kernel flags the pieces that start a run, a scan numbers them, depth_runs_kernel writes a run's start and depth from its first
//                piece and its end from its last; depth_runlen_kernel: a run's length, length * depth and its (contig, depth) key.
//   contigs      exclusive scans of the lengths and of length * depth in start order; one sort of the runs by (contig, depth) and a scan of their lengths;
//                depth_contig_kernel: one thread per listed contig, all counters from binary searches into these (mmdp::contig_stats).
//   windows      depth_window_kernel: one thread per window: its contig from a binary search into win_off, its runs from two more (mmdp::window_sums).
// The listed contigs, their lengths and win_off come from the host, which has to read every interval for its checks anyway.  No kernel here waits for another
// workgroup and none uses an atomic; every loop runs over the steps of a binary search or over the thresholds (8 at most, checked by the host).
#include "mm_depth.hpp"
#include "mm_depth_core.hpp"
#include "mm_keytable.hpp"
#include "mm_prims.hpp"
#include <string>

namespace mm {

__global__ void __launch_bounds__(256) depth_breaks_kernel(const uint64_t* __restrict__ starts, const uint64_t* __restrict__ ends, int64_t n, uint64_t* __restrict__ bk) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { bk[i] = starts[i]; bk[n + i] = mmdp::end_break(ends[i]); }
}
// head[i]: sorted[i] is the first of its equals; head[n] = 0 for the scan's total
__global__ void __launch_bounds__(256) depth_unique_kernel(const uint64_t* __restrict__ sorted, int64_t n, uint8_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) head[i] = i == 0 || sorted[i] != sorted[i - 1] ? 1 : 0;
  else if (i == n) head[i] = 0;
}
__global__ void __launch_bounds__(256) depth_compact_kernel(const uint64_t* __restrict__ sorted, const uint8_t* __restrict__ head, const int64_t* __restrict__ pos, int64_t n,
                                                            uint64_t* __restrict__ ub) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && head[i]) ub[pos[i]] = sorted[i];
}
__global__ void __launch_bounds__(256) depth_piece_kernel(const uint64_t* __restrict__ ub, int64_t m, const uint64_t* __restrict__ starts, const uint64_t* __restrict__ ends, int64_t n_iv,
                                                          uint32_t* __restrict__ pd) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < m) pd[j] = mmdp::piece_depth(starts, ends, n_iv, ub[j]);
}
// rh[j]: piece j starts a run; rh[m] = 0 for the scan's total
__global__ void __launch_bounds__(256) depth_runhead_kernel(const uint64_t* __restrict__ ub, const uint32_t* __restrict__ pd, int64_t m, uint8_t* __restrict__ rh) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < m) rh[j] = mmdp::run_head(j > 0, j > 0 ? ub[j - 1] : 0, j > 0 ? pd[j - 1] : 0, ub[j], pd[j]) ? 1 : 0;
  else if (j == m) rh[j] = 0;
}
// rpos: the exclusive sums of rh.  A piece of depth >= 1 lies in run rpos[j] + rh[j] - 1 (a piece that heads none has a head before it on its contig);
// the run's first piece writes its start and depth, its last piece the end: the next breakpoint, which exists (mm_depth_core.hpp, "pieces").
__global__ void __launch_bounds__(256) depth_runs_kernel(const uint64_t* __restrict__ ub, const uint32_t* __restrict__ pd, const uint8_t* __restrict__ rh, const int64_t* __restrict__ rpos,
                                                         int64_t m, int64_t n_runs, uint64_t* __restrict__ rstart, uint64_t* __restrict__ rend, uint32_t* __restrict__ rdepth) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m || pd[j] == 0) return;
  const int64_t r = rpos[j] + rh[j] - 1;
  if (r < 0 || r >= n_runs) return;
  if (rh[j]) { rstart[r] = ub[j]; rdepth[r] = pd[j]; }
  if (j + 1 < m && mmdp::run_tail(pd[j], true, pd[j + 1])) rend[r] = ub[j + 1];
}
// per run its length, length * depth and (contig, depth) key; entry n_runs of the two sums: 0 for the scans' totals
__global__ void __launch_bounds__(256) depth_runlen_kernel(const uint64_t* __restrict__ rstart, const uint64_t* __restrict__ rend, const uint32_t* __restrict__ rdepth, int64_t n_runs,
                                                           uint64_t* __restrict__ len, uint64_t* __restrict__ sum, uint64_t* __restrict__ dkey) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < n_runs) {
    const uint64_t l = rend[r] - rstart[r];
    len[r] = l; sum[r] = l * rdepth[r]; dkey[r] = (rstart[r] & ~mmdp::POS_MASK) | rdepth[r];
  } else if (r == n_runs) { len[r] = 0; sum[r] = 0; }
}
// stats[(STATS + T.n) * j ..]: the counters of the j-th listed contig
__global__ void __launch_bounds__(256) depth_contig_kernel(const int32_t* __restrict__ listed, const int64_t* __restrict__ llen, int64_t n_listed, const uint64_t* __restrict__ starts,
                                                           int64_t n_iv, mmdp::Runs R, mmdp::RunsByDepth D, mmdp::Thresholds T, int64_t* __restrict__ stats) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_listed) return;
  int64_t out[mmdp::STATS + mmdp::MAX_THRESHOLDS];
  mmdp::contig_stats(listed[j], llen[j], starts, n_iv, R, D, T, out);
  for (int k = 0; k < mmdp::STATS + T.n; ++k) stats[(int64_t)(mmdp::STATS + T.n) * j + k] = out[k];
}
__global__ void __launch_bounds__(256) depth_window_kernel(const int32_t* __restrict__ listed, const int64_t* __restrict__ llen, const uint64_t* __restrict__ win_off, int64_t n_listed,
                                                           int64_t n_windows, int64_t window, mmdp::Runs R, int64_t* __restrict__ sum, int64_t* __restrict__ covered) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n_windows) return;
  const int64_t j = mmdp::window_contig(win_off, n_listed, w);
  int64_t a, b, s, n;
  mmdp::window_span(llen[j], window, w - (int64_t)win_off[j], &a, &b);
  mmdp::window_sums(listed[j], a, b, R, &s, &n);
  sum[w] = s; covered[w] = n;
}

void depth_profile_run(mm_ctx* ctx, const DepthIn& in, DepthResult* out) {
  const std::string who = "mm_depth_profile: ";
  // before anything is launched: every later index is inside its array
  MM_REQUIRE(in.n_contigs >= 0 && in.n_contigs <= mmdp::MAX_CONTIGS, MM_ERR_ARG, who + "a negative number of contigs, or more than 2^29 contigs");
  MM_REQUIRE(in.n_iv >= 0 && in.n_iv < ((int64_t)1 << 31), in.n_iv < 0 ? MM_ERR_ARG : MM_ERR_LIMIT, who + "a negative number of intervals, or 2^31 or more (a depth is a 32-bit sum)");
  MM_REQUIRE((in.n_contigs == 0 || in.contig_len) && (in.n_iv == 0 || (in.iv_contig && in.iv_first && in.iv_last)) && (in.n_thresholds <= 0 || in.thresholds), MM_ERR_ARG,
             who + "a null array");
  MM_REQUIRE(in.window >= 1, MM_ERR_ARG, who + "window " + std::to_string(in.window) + " is less than 1");
  MM_REQUIRE(mmdp::thresholds_ok(in.n_thresholds, in.thresholds), MM_ERR_ARG, who + "more than 8 thresholds, a threshold below 1, or thresholds that are not strictly ascending");
  for (int64_t c = 0; c < in.n_contigs; ++c)
    MM_REQUIRE(mmdp::length_ok(in.contig_len[c]), MM_ERR_ARG, who + "the length of contig " + std::to_string(c) + " lies outside [1, 2^29)");
  for (int64_t i = 0; i < in.n_iv; ++i)
    MM_REQUIRE(mmdp::interval_ok(in.iv_contig[i], in.iv_first[i], in.iv_last[i], in.n_contigs, in.contig_len), MM_ERR_ARG,
               who + "interval " + std::to_string(i) + " is empty or lies outside its contig");
  *out = DepthResult{};
  out->n_thresholds = in.n_thresholds;
  mmdp::Thresholds T{in.n_thresholds, {}};
  for (int32_t k = 0; k < in.n_thresholds; ++k) T.t[k] = in.thresholds[k];
  std::vector<int32_t> listed(in.iv_contig, in.iv_contig + in.n_iv);   // the contigs with an interval, ascending
  std::sort(listed.begin(), listed.end());
  listed.erase(std::unique(listed.begin(), listed.end()), listed.end());
  const size_t nl = listed.size();
  std::vector<int64_t> llen(nl); std::vector<uint64_t> win_off(nl + 1, 0);
  for (size_t j = 0; j < nl; ++j) {
    llen[j] = in.contig_len[listed[j]];
    win_off[j + 1] = win_off[j] + (uint64_t)mmdp::window_count(llen[j], in.window);
    MM_REQUIRE(win_off[j + 1] <= (uint64_t)mmdp::MAX_WINDOWS, MM_ERR_ARG, who + "more than 2^31 - 1 windows at window " + std::to_string(in.window) + " (reached at contig " +
               std::to_string(listed[j]) + "): take a larger window");
  }
  if (in.n_iv == 0) return;                                        // nothing is launched

  hipStream_t st = ctx->stream;
  const bool timing = getenv("MM_DEPTH_TIMING") != nullptr;
  StageClock<5> clk(timing, st);                                   // intervals, breakpoints, runs, contigs, windows (each with its way to the host)
  const int64_t n = in.n_iv, n2 = 2 * n, n_windows = (int64_t)win_off[nl];
  const size_t v = (size_t)n, v2 = (size_t)n2;
  const int bits = 32 + contig_bits(in.n_contigs);
  DBuf<uint8_t> tmp;

  clk.start();
  SortedIntervals iv;
  iv.starts.alloc(v); iv.end_of.alloc(v); iv.ends.alloc(v);
  sorted_interval_keys(tmp, FinishIn{0, nullptr, nullptr, nullptr, n, in.iv_contig, in.iv_first, in.iv_last, 0, 0.0}, bits, st, iv);
  clk.stop(0);

  clk.start();
  DBuf<uint64_t> d_bk(v2), d_sbk(v2), d_ub(v2); DBuf<uint8_t> d_head(v2 + 1); DBuf<int64_t> d_pos(v2 + 1);
  depth_breaks_kernel<<<dim3(flat_grid(n)), dim3(256), 0, st>>>(iv.starts.p, iv.ends.p, n, d_bk.p); MM_KERNEL_CHECK();
  sort_keys(tmp, d_bk.p, d_sbk.p, v2, 0, bits, st);
  depth_unique_kernel<<<dim3(flat_grid(n2 + 1)), dim3(256), 0, st>>>(d_sbk.p, n2, d_head.p); MM_KERNEL_CHECK();
  exclusive_scan(tmp, d_head.p, d_pos.p, v2 + 1, st);
  depth_compact_kernel<<<dim3(flat_grid(n2)), dim3(256), 0, st>>>(d_sbk.p, d_head.p, d_pos.p, n2, d_ub.p); MM_KERNEL_CHECK();
  int64_t m = 0;
  d_pos.download(&m, 1, st, v2);
  MM_HIP(mm::stream_sync(st));
  MM_REQUIRE(m >= 2 && m <= n2, MM_ERR_DEVICE, who + "the unique breakpoints are fewer than 2 or more than the interval ends");
  DBuf<uint32_t> d_pd((size_t)m);
  depth_piece_kernel<<<dim3(flat_grid(m)), dim3(256), 0, st>>>(d_ub.p, m, iv.starts.p, iv.ends.p, n, d_pd.p); MM_KERNEL_CHECK();
  clk.stop(1);

  clk.start();
  DBuf<uint8_t> d_rh((size_t)m + 1); DBuf<int64_t> d_rpos((size_t)m + 1);
  depth_runhead_kernel<<<dim3(flat_grid(m + 1)), dim3(256), 0, st>>>(d_ub.p, d_pd.p, m, d_rh.p); MM_KERNEL_CHECK();
  exclusive_scan(tmp, d_rh.p, d_rpos.p, (size_t)m + 1, st);
  int64_t n_runs = 0;
  d_rpos.download(&n_runs, 1, st, (size_t)m);
  MM_HIP(mm::stream_sync(st));
  MM_REQUIRE(n_runs >= 1 && n_runs < m, MM_ERR_DEVICE, who + "the runs are fewer than 1 or not fewer than the breakpoints");
  const size_t nr = (size_t)n_runs;
  DBuf<uint64_t> d_rstart(nr), d_rend(nr), d_len(nr + 1), d_sum(nr + 1), d_dkey(nr); DBuf<uint32_t> d_rdepth(nr);
  d_rend.zero(st);
  depth_runs_kernel<<<dim3(flat_grid(m)), dim3(256), 0, st>>>(d_ub.p, d_pd.p, d_rh.p, d_rpos.p, m, n_runs, d_rstart.p, d_rend.p, d_rdepth.p); MM_KERNEL_CHECK();
  depth_runlen_kernel<<<dim3(flat_grid(n_runs + 1)), dim3(256), 0, st>>>(d_rstart.p, d_rend.p, d_rdepth.p, n_runs, d_len.p, d_sum.p, d_dkey.p); MM_KERNEL_CHECK();
  const std::vector<uint64_t> rstart = d_rstart.to_host(st), rend = d_rend.to_host(st);
  out->run_depth = d_rdepth.to_host(st);
  out->run_contig.resize(nr); out->run_start.resize(nr); out->run_end.resize(nr);
  for (size_t r = 0; r < nr; ++r) {
    MM_REQUIRE(rend[r] > rstart[r] && mmdp::key_contig(rend[r]) == mmdp::key_contig(rstart[r]) && out->run_depth[r] > 0, MM_ERR_DEVICE, who + "run " + std::to_string(r) + " has no end on its contig");
    out->run_contig[r] = (int32_t)mmdp::key_contig(rstart[r]); out->run_start[r] = mmdp::key_pos(rstart[r]); out->run_end[r] = mmdp::key_pos(rend[r]);
  }
  clk.stop(2);

  clk.start();
  DBuf<uint64_t> d_plen(nr + 1), d_psum(nr + 1), d_sdkey(nr), d_slen(nr + 1), d_dlen(nr + 1);
  exclusive_scan(tmp, d_len.p, d_plen.p, nr + 1, st);
  exclusive_scan(tmp, d_sum.p, d_psum.p, nr + 1, st);
  MM_HIP(hipMemsetAsync(d_slen.p + nr, 0, sizeof(uint64_t), st));  // ([n_runs] = 0: the scan's total)
  sort_pairs(tmp, d_dkey.p, d_sdkey.p, d_len.p, d_slen.p, nr, 0, bits, st);
  exclusive_scan(tmp, d_slen.p, d_dlen.p, nr + 1, st);
  const mmdp::Runs R{n_runs, d_rstart.p, d_rend.p, d_rdepth.p, d_plen.p, d_psum.p};
  const mmdp::RunsByDepth D{d_sdkey.p, d_dlen.p};
  const size_t per = (size_t)(mmdp::STATS + in.n_thresholds);
  DBuf<int32_t> d_listed(nl); DBuf<int64_t> d_llen(nl), d_stats(per * nl); DBuf<uint64_t> d_win_off(nl + 1);
  d_listed.upload(listed.data(), nl, st); d_llen.upload(llen.data(), nl, st); d_win_off.upload(win_off.data(), nl + 1, st);
  depth_contig_kernel<<<dim3(flat_grid((int64_t)nl)), dim3(256), 0, st>>>(d_listed.p, d_llen.p, (int64_t)nl, iv.starts.p, n, R, D, T, d_stats.p); MM_KERNEL_CHECK();
  out->stats = d_stats.to_host(st);
  clk.stop(3);

  clk.start();
  DBuf<int64_t> d_wsum((size_t)n_windows), d_wcov((size_t)n_windows);
  depth_window_kernel<<<dim3(flat_grid(n_windows)), dim3(256), 0, st>>>(d_listed.p, d_llen.p, d_win_off.p, (int64_t)nl, n_windows, in.window, R, d_wsum.p, d_wcov.p); MM_KERNEL_CHECK();
  out->win_sum = d_wsum.to_host(st); out->win_covered = d_wcov.to_host(st);
  clk.stop(4);

  out->contig = listed;
  out->win_off.assign(win_off.begin(), win_off.end());
  if (timing)
    fprintf(stderr, "MM_DEPTH_TIMING profile: intervals %.3f breakpoints %.3f runs %.3f contigs %.3f windows %.3f ms; %lld intervals, %lld breakpoints, %lld runs, %zu contigs, "
            "%lld windows\n", clk.ms[0], clk.ms[1], clk.ms[2], clk.ms[3], clk.ms[4], (long long)n, (long long)m, (long long)n_runs, nl, (long long)n_windows);
}

}  // namespace mm
