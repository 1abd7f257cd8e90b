// Sorted runs of BAM records merged into one coordinate-sorted stream, and its BAI index (mm_bam_sorter_*; DESIGN.md section 1, "Sorted BAM"; the
// definitions: mm_bam_sort_core.hpp, the text the host test runs).
//   add_run  the host walks the run's BSIZE / ISIZE chain once and checks the records' keys; the members stay where the caller has them.
//   plan     one stable radix sort of all (sort_key, record) pairs, the sizes gathered in that order, an exclusive scan: every record's offset in the
//            output stream.  The order and the offsets stay on the device and come to the host once.
//   window   output bytes [w W, (w + 1) W).  The records that reach into them are a contiguous range of every run; the host finds, per run, the members
//            that cover the needed bytes, bgzf_inflate_resident inflates those into one device buffer (at most W and two members per run), and
//            bam_gather_kernel copies: one wavefront per SPAN bytes of output finds the first record that reaches into them (a binary search over the
//            offsets) and moves each record's part that lies inside (copy_bytes: 16-byte, or shifted 32-bit words where the residues differ), so a long
//            record is cut at every SPAN and no wave walks more.  bgzf_deflate_resident makes the members; only they come to the host.
//   index    per record in file order vs, ve, bin_key and end_key; bins: a stable sort by bin_key with the ordinal as value, chunk heads, a scan, a
//            compaction; linear index: an inclusive maximum scan of end_key and a binary search per window.  The host serialises (bai_bytes).
// No kernel here has an atomic, a barrier between workgroups or a loop that waits for another workgroup.
#include "mm_bam_sort.hpp"
#include "mm_bam.hpp"
#include "mm_bam_sort_core.hpp"
#include "mm_deflate.hpp"
#include "mm_inflate.hpp"
#include "mm_jobs_dev.hpp"
#include "mm_prims.hpp"
#include <string>

namespace mm {

static_assert(mmbs::MEMBER_RAW == (int64_t)mmd::BLOCK_IN && BAM_GROUP_BYTES == mmd::LAUNCH_BLOCKS * mmbs::MEMBER_RAW, "a window is one launch of the deflate kernel at most");

__global__ void __launch_bounds__(256) bam_sort_key_kernel(const int32_t* __restrict__ ref, const int32_t* __restrict__ pos, int64_t n, uint64_t* __restrict__ key) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < n) key[g] = mmbs::sort_key(ref[g], pos[g]);
}
__global__ void __launch_bounds__(256) bam_sort_take_kernel(const int64_t* __restrict__ perm, const int64_t* __restrict__ src, int64_t n, int64_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[perm[i]];
}

// The window's bytes [lo, hi) of the stream to out[0, hi - lo).  in + delta[run] is where byte 0 of the run's inflated bytes would lie: the members that
// hold the needed bytes are there.  Reads in[] within the aligned words around each piece (the buffer has 16 bytes behind its last member).
__global__ void __launch_bounds__(64) bam_gather_kernel(const int64_t* __restrict__ out_off, const int64_t* __restrict__ perm, const int64_t* __restrict__ src_off,
                                                        const int32_t* __restrict__ run_of, const int64_t* __restrict__ delta, int64_t n, int64_t lo, int64_t hi,
                                                        const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
  const int64_t c_lo = lo + (int64_t)blockIdx.x * mmbs::SPAN, c_hi = c_lo + mmbs::SPAN < hi ? c_lo + mmbs::SPAN : hi;
  if (c_lo >= hi) return;
  WaveLanes p;
  for (int64_t i = mmbs::upper_record(out_off, n, c_lo); i < n && out_off[i] < c_hi; ++i) {
    const int64_t g = perm[i];
    const mmbs::Piece pc = mmbs::clip(out_off[i], out_off[i + 1] - out_off[i], src_off[g], c_lo, c_hi);
    mmbs::copy_bytes(p, in + delta[run_of[g]] + pc.src, out + (c_lo - lo) + pc.dst, pc.len);
  }
}

// per record in file order: its virtual offsets and the two keys of the index
__global__ void __launch_bounds__(256) bam_index_rec_kernel(const int64_t* __restrict__ perm, const int64_t* __restrict__ out_off, const int64_t* __restrict__ member_at,
                                                            const int32_t* __restrict__ ref, const int32_t* __restrict__ pos, const int32_t* __restrict__ end, int64_t n,
                                                            uint64_t* __restrict__ vs, uint64_t* __restrict__ ve, uint64_t* __restrict__ bkey, uint64_t* __restrict__ ekey) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t g = perm[i];
  vs[i] = mmbs::voff(out_off[i], member_at, out_off[n]); ve[i] = mmbs::voff(out_off[i + 1], member_at, out_off[n]);
  bkey[i] = mmbs::bin_key(ref[g], mmb::reg2bin(pos[g], end[g])); ekey[i] = mmbs::end_key(ref[g], end[g]);
}
__global__ void __launch_bounds__(256) bam_index_head_kernel(const uint64_t* __restrict__ key, const int64_t* __restrict__ ord, int64_t n, int64_t* __restrict__ head) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) head[j] = mmbs::chunk_head(key, ord, j);
}
// the chunks compacted: at[j] is the number of heads before j
__global__ void __launch_bounds__(256) bam_index_chunk_kernel(const uint64_t* __restrict__ key, const int64_t* __restrict__ ord, const int64_t* __restrict__ head,
                                                              const int64_t* __restrict__ at, const uint64_t* __restrict__ vs, const uint64_t* __restrict__ ve, int64_t n,
                                                              uint64_t* __restrict__ ckey, uint64_t* __restrict__ cvs, uint64_t* __restrict__ cve) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  if (head[j]) { ckey[at[j]] = key[j]; cvs[at[j]] = vs[ord[j]]; }
  if (j == n - 1 || head[j + 1]) cve[at[j] + head[j] - 1] = ve[ord[j]];
}
// per reference: the largest end, the first record's vs and the last one's ve (0 where it has no record)
__global__ void __launch_bounds__(256) bam_index_ref_kernel(const int64_t* __restrict__ ref_start, int32_t n_ref, const uint64_t* __restrict__ M, const uint64_t* __restrict__ vs,
                                                            const uint64_t* __restrict__ ve, int32_t* __restrict__ max_end, uint64_t* __restrict__ first_vs, uint64_t* __restrict__ last_ve) {
  const int32_t r = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (r >= n_ref) return;
  const int64_t a = ref_start[r], b = ref_start[r + 1];
  max_end[r] = b > a ? (int32_t)(uint32_t)M[b - 1] : 0; first_vs[r] = b > a ? vs[a] : 0; last_ve[r] = b > a ? ve[b - 1] : 0;
}
__global__ void __launch_bounds__(256) bam_index_linear_kernel(const int64_t* __restrict__ ref_start, const int64_t* __restrict__ win_off, int32_t n_ref, const uint64_t* __restrict__ M,
                                                               const uint64_t* __restrict__ vs, uint64_t* __restrict__ ioff) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= win_off[n_ref]) return;
  const int32_t r = (int32_t)mmbs::first_above<int64_t>(win_off + 1, 0, n_ref, w);   // the reference whose windows hold w
  const int64_t a = ref_start[r], b = ref_start[r + 1];
  const int64_t i = mmbs::first_above<uint64_t>(M, a, b, mmbs::end_key(r, (int32_t)((w - win_off[r]) << mmbs::LINEAR_SHIFT)));
  ioff[w] = i < b ? vs[i] : 0;                                     // (i < b: the reference's largest end lies behind its last window's start)
}

void bam_sorter_init(BamSorter& s, int32_t n_ref, const int32_t* ref_len, int64_t window_bytes) {
  MM_REQUIRE(n_ref >= 0 && (n_ref == 0 || ref_len), MM_ERR_ARG, "mm_bam_sorter_create: a negative n_ref or a null array");
  for (int32_t r = 0; r < n_ref; ++r) {
    MM_REQUIRE(ref_len[r] >= 0, MM_ERR_ARG, "mm_bam_sorter_create: reference " + std::to_string(r) + " has a negative length");
    MM_REQUIRE(ref_len[r] < mmbs::COORD_END, MM_ERR_ARG, "mm_bam_sorter_create: reference " + std::to_string(r) + " has 2^29 bases or more: BAI does not hold its coordinates");
  }
  MM_REQUIRE(window_bytes >= 0 && window_bytes % mmbs::MEMBER_RAW == 0 && window_bytes <= BAM_GROUP_BYTES, MM_ERR_ARG,
             "mm_bam_sorter_create: window_bytes is not 0 or a multiple of 65280 up to " + std::to_string(BAM_GROUP_BYTES));
  s.ref_len.assign(ref_len, ref_len + n_ref);
  s.window = window_bytes ? window_bytes : BAM_GROUP_BYTES;
}

// the run's members: MM_ERR_DATA for a chain that breaks
static void walk_members(BamSortRun& run, int64_t bytes, const std::string& who) {
  run.mem_raw.assign(1, 0);
  for (int64_t at = 0; at < bytes;) {
    const uint8_t* m = run.bgzf + at;
    const std::string where = who + ": member " + std::to_string(run.mem_off.size()) + " at byte " + std::to_string(at);
    MM_REQUIRE(at + 26 <= bytes && m[0] == 0x1f && m[1] == 0x8b && m[2] == 8 && m[3] == 4 && m[10] == 6 && m[11] == 0 && m[12] == 'B' && m[13] == 'C' && m[14] == 2 && m[15] == 0,
               MM_ERR_DATA, where + " is not a BGZF member");
    const int64_t len = (int64_t)(m[16] | m[17] << 8) + 1;
    MM_REQUIRE(len >= 26 && at + len <= bytes, MM_ERR_DATA, where + " runs past the run's end");
    const uint32_t isize = mmi::rd32(m + len - 4);
    MM_REQUIRE(isize <= mmi::MAX_ISIZE, MM_ERR_DATA, where + " says it inflates to more than 65536 bytes");
    run.mem_off.push_back(at); run.mem_len.push_back((int32_t)len); run.mem_raw.push_back(run.mem_raw.back() + isize);
    at += len;
  }
}

void bam_sorter_add_run(BamSorter& s, const uint8_t* bgzf, int64_t bgzf_bytes, int64_t n, const int64_t* raw_off, const int32_t* ref_id, const int32_t* pos, const int32_t* end) {
  const std::string who = "mm_bam_sorter_add_run: run " + std::to_string(s.runs.size());
  MM_REQUIRE(!s.planned, MM_ERR_STATE, who + " comes after the plan");
  MM_REQUIRE(bgzf_bytes >= 0 && n >= 0 && raw_off && (bgzf_bytes == 0 || bgzf) && (n == 0 || (ref_id && pos && end)), MM_ERR_ARG, who + ": a negative size or a null array");
  BamSortRun run; run.bgzf = bgzf; run.n = n;
  walk_members(run, bgzf_bytes, who);
  MM_REQUIRE(raw_off[0] == 0 && raw_off[n] == run.mem_raw.back(), MM_ERR_ARG,
             who + ": record " + std::to_string(n) + ": raw_off ends at " + std::to_string(raw_off[n]) + ", the members inflate to " + std::to_string(run.mem_raw.back()) + " bytes (or raw_off[0] is not 0)");
  const int64_t n_ref = (int64_t)s.ref_len.size();
  auto rec = [&](int64_t i) { return who + ": record " + std::to_string(i); };
  for (int64_t i = 0; i < n; ++i) {
    MM_REQUIRE(raw_off[i + 1] > raw_off[i], MM_ERR_ARG, rec(i) + ": raw_off does not rise");
    MM_REQUIRE(ref_id[i] >= 0 && ref_id[i] < n_ref, MM_ERR_ARG, rec(i) + ": ref_id is out of range");
    MM_REQUIRE(pos[i] >= 0, MM_ERR_ARG, rec(i) + ": pos is negative");
    MM_REQUIRE(end[i] > pos[i] && end[i] <= s.ref_len[(size_t)ref_id[i]], MM_ERR_ARG, rec(i) + ": end is not behind pos, or lies past the contig's end");
    MM_REQUIRE(i == 0 || mmbs::sort_key(ref_id[i - 1], pos[i - 1]) <= mmbs::sort_key(ref_id[i], pos[i]), MM_ERR_ARG, rec(i) + ": the run is not sorted by (ref_id, pos)");
  }
  for (int64_t i = 0; i < n; ++i) {
    s.ref.push_back(ref_id[i]); s.pos.push_back(pos[i]); s.end.push_back(end[i]); s.run_of.push_back((int32_t)s.runs.size());
    s.src_off.push_back(raw_off[i]); s.size.push_back(raw_off[i + 1] - raw_off[i]);
  }
  s.n += n;
  s.runs.push_back(std::move(run));
}

void bam_sorter_plan(mm_ctx* ctx, BamSorter& s) {
  MM_REQUIRE(!s.planned, MM_ERR_STATE, "mm_bam_sorter_plan: called twice");
  s.planned = true; s.out_off.assign(1, 0);
  if (s.n == 0) return;
  hipStream_t st = ctx->stream;
  const size_t k = (size_t)s.n;
  DBuf<int32_t> d_ref(k), d_pos(k); DBuf<uint64_t> d_key(k), d_sorted(k); DBuf<int64_t> d_iota(k), d_size(k), d_sized(k + 1);
  s.d_perm.alloc(k); s.d_out_off.alloc(k + 1); s.d_src_off.alloc(k); s.d_run.alloc(k);
  d_ref.upload(s.ref.data(), k, st); d_pos.upload(s.pos.data(), k, st); d_size.upload(s.size.data(), k, st);
  s.d_src_off.upload(s.src_off.data(), k, st); s.d_run.upload(s.run_of.data(), k, st);
  bam_sort_key_kernel<<<dim3(flat_grid(s.n)), dim3(256), 0, st>>>(d_ref.p, d_pos.p, s.n, d_key.p);
  MM_KERNEL_CHECK();
  fill_iota(d_iota.p, s.n, st);
  sort_pairs(s.tmp, d_key.p, d_sorted.p, d_iota.p, s.d_perm.p, k, 0, 32 + bits_for(s.ref_len.size()), st);   // (stable: ties stay in (run, index) order)
  d_sized.zero(st);
  bam_sort_take_kernel<<<dim3(flat_grid(s.n)), dim3(256), 0, st>>>(s.d_perm.p, d_size.p, s.n, d_sized.p);
  MM_KERNEL_CHECK();
  exclusive_scan(s.tmp, d_sized.p, s.d_out_off.p, k + 1, st);
  s.perm = s.d_perm.to_host(st); s.out_off = s.d_out_off.to_host(st);
  s.stream_bytes = s.out_off[k];
}

// what a window needs of the runs: the members to inflate and where, and every run's delta; returns the bytes of d_in
struct WindowNeed { std::vector<const uint8_t*> block; std::vector<int32_t> len, run, member; std::vector<int64_t> at, delta; int64_t bytes = 0; };
static WindowNeed window_need(const BamSorter& s, int64_t lo, int64_t hi) {
  const size_t n_runs = s.runs.size();
  std::vector<int64_t> a(n_runs, INT64_MAX), b(n_runs, -1);
  for (int64_t i = mmbs::upper_record(s.out_off.data(), s.n, lo); i < s.n && s.out_off[(size_t)i] < hi; ++i) {
    const size_t g = (size_t)s.perm[(size_t)i], r = (size_t)s.run_of[g];
    const mmbs::Piece pc = mmbs::clip(s.out_off[(size_t)i], s.size[g], s.src_off[g], lo, hi);
    a[r] = std::min(a[r], pc.src); b[r] = std::max(b[r], pc.src + pc.len);
  }
  WindowNeed need; need.delta.assign(n_runs, 0);
  for (size_t r = 0; r < n_runs; ++r) {
    if (b[r] <= a[r]) continue;
    const BamSortRun& run = s.runs[r];
    const int64_t n_mem = (int64_t)run.mem_off.size();
    const int64_t m0 = mmbs::first_above<int64_t>(run.mem_raw.data() + 1, 0, n_mem, a[r]), m1 = mmbs::first_above<int64_t>(run.mem_raw.data() + 1, 0, n_mem, b[r] - 1) + 1;
    need.delta[r] = need.bytes - run.mem_raw[(size_t)m0];
    for (int64_t m = m0; m < m1; ++m) {
      need.block.push_back(run.bgzf + run.mem_off[(size_t)m]); need.len.push_back(run.mem_len[(size_t)m]); need.run.push_back((int32_t)r); need.member.push_back((int32_t)m);
      need.at.push_back(need.bytes + run.mem_raw[(size_t)m] - run.mem_raw[(size_t)m0]);
    }
    need.bytes = (need.bytes + run.mem_raw[(size_t)m1] - run.mem_raw[(size_t)m0] + 31) & ~(int64_t)15;   // (the next run starts on 16 bytes, 16 behind this one)
  }
  return need;
}

void bam_sorter_window(mm_ctx* ctx, BamSorter& s, int64_t w) {
  MM_REQUIRE(s.planned, MM_ERR_STATE, "mm_bam_sorter_window: there is no plan yet");
  MM_REQUIRE(w == s.next_window && w < bam_sorter_windows(s), MM_ERR_STATE, "mm_bam_sorter_window: window " + std::to_string(w) + " is not the next one, " + std::to_string(s.next_window));
  hipStream_t st = ctx->stream;
  const int64_t lo = w * s.window, hi = std::min(s.stream_bytes, lo + s.window), bytes = hi - lo;
  const WindowNeed need = window_need(s, lo, hi);
  if (s.d_in.n < (size_t)need.bytes + 16) s.d_in.alloc((size_t)need.bytes + 16);
  if (s.d_out.n < (size_t)std::min(s.window, s.stream_bytes) + 16) s.d_out.alloc((size_t)std::min(s.window, s.stream_bytes) + 16);
  std::vector<int32_t> status(need.block.size(), 0);
  StageClock<3> clk(getenv("MM_BAM_SORT_TIMING") != nullptr, st);  // inflate (with the members' upload), gather, deflate (with the members' way to the host)
  clk.start();
  const int64_t bad = bgzf_inflate_resident(ctx, need.block.data(), need.len.data(), (int32_t)need.block.size(), s.d_in.p, need.bytes, need.at.data(), status.data());
  for (size_t i = 0; bad && i < status.size(); ++i)
    MM_REQUIRE(status[i] == 0, MM_ERR_DATA, "mm_bam_sorter_window: run " + std::to_string(need.run[i]) + ": member " + std::to_string(need.member[i]) + " does not inflate (status " + std::to_string(status[i]) + ")");
  clk.stop(0);
  clk.start();
  DBuf<int64_t> d_delta(need.delta.size());
  d_delta.upload(need.delta.data(), need.delta.size(), st);
  bam_gather_kernel<<<dim3((unsigned)ceil_div(bytes, mmbs::SPAN)), dim3(64), 0, st>>>(s.d_out_off.p, s.d_perm.p, s.d_src_off.p, s.d_run.p, d_delta.p, s.n, lo, hi, s.d_in.p, s.d_out.p);
  MM_KERNEL_CHECK();
  clk.stop(1);
  clk.start();
  const int64_t nb = mmd::n_blocks_of(bytes);
  uint8_t* const down = (uint8_t*)ctx->pinned_at_least((size_t)nb * mmd::MEMBER_MAX);
  std::vector<int32_t> sizes((size_t)nb, 0);
  bgzf_deflate_resident(ctx, s.d_out.p, bytes, nb, down, sizes.data());
  clk.stop(2);
  if (clk.on)
    fprintf(stderr, "MM_BAM_SORT_TIMING window %lld: inflate %.3f gather %.3f deflate %.3f ms; %zu members in (%lld B inflated), %lld B out\n", (long long)w, clk.ms[0], clk.ms[1], clk.ms[2],
            need.block.size(), (long long)need.bytes, (long long)bytes);
  s.product.clear();
  for (int64_t m = 0; m < nb; ++m) {
    MM_REQUIRE(sizes[(size_t)m] >= 26 && sizes[(size_t)m] <= (int32_t)mmd::BLOCK_IN + 31, MM_ERR_DEVICE, "mm_bam_sorter_window: a member's size is out of range");
    s.product.insert(s.product.end(), down + m * mmd::MEMBER_MAX, down + m * mmd::MEMBER_MAX + sizes[(size_t)m]);
    s.member_bytes.push_back(sizes[(size_t)m]);
  }
  ++s.next_window;
}

// the chunks of the bins on the device; fills the vectors
static void index_bins(BamSorter& s, uint64_t* d_bkey, const uint64_t* d_vs, const uint64_t* d_ve, hipStream_t st, std::vector<uint64_t>* ckey, std::vector<uint64_t>* cvs, std::vector<uint64_t>* cve) {
  const size_t k = (size_t)s.n;
  DBuf<uint64_t> d_skey(k), d_ckey(k), d_cvs(k), d_cve(k); DBuf<int64_t> d_iota(k), d_ord(k), d_head(k + 1), d_at(k + 1);
  fill_iota(d_iota.p, s.n, st);
  sort_pairs(s.tmp, d_bkey, d_skey.p, d_iota.p, d_ord.p, k, 0, 16 + bits_for(s.ref_len.size()), st);
  d_head.zero(st);
  bam_index_head_kernel<<<dim3(flat_grid(s.n)), dim3(256), 0, st>>>(d_skey.p, d_ord.p, s.n, d_head.p);
  MM_KERNEL_CHECK();
  exclusive_scan(s.tmp, d_head.p, d_at.p, k + 1, st);
  bam_index_chunk_kernel<<<dim3(flat_grid(s.n)), dim3(256), 0, st>>>(d_skey.p, d_ord.p, d_head.p, d_at.p, d_vs, d_ve, s.n, d_ckey.p, d_cvs.p, d_cve.p);
  MM_KERNEL_CHECK();
  const size_t n_chunks = (size_t)d_at.to_host(st)[k];
  *ckey = d_ckey.to_host(st, n_chunks); *cvs = d_cvs.to_host(st, n_chunks); *cve = d_cve.to_host(st, n_chunks);
}

void bam_sorter_index(mm_ctx* ctx, BamSorter& s, int64_t header_bytes) {
  MM_REQUIRE(s.planned && s.next_window == bam_sorter_windows(s), MM_ERR_STATE, "mm_bam_sorter_index: the windows are not all made");
  MM_REQUIRE(header_bytes >= 0, MM_ERR_ARG, "mm_bam_sorter_index: a negative header_bytes");
  const int32_t n_ref = (int32_t)s.ref_len.size();
  std::vector<int64_t> ref_start((size_t)n_ref + 1, 0), win_off((size_t)n_ref + 1, 0);
  for (int32_t r : s.ref) ++ref_start[(size_t)r + 1];
  for (int32_t r = 0; r < n_ref; ++r) ref_start[(size_t)r + 1] += ref_start[(size_t)r];
  std::vector<uint64_t> first_vs((size_t)n_ref, 0), last_ve((size_t)n_ref, 0), ckey, cvs, cve, ioff;
  if (s.n > 0) {
    hipStream_t st = ctx->stream;
    const size_t k = (size_t)s.n;
    std::vector<int64_t> member_at(1, header_bytes);
    for (int32_t b : s.member_bytes) member_at.push_back(member_at.back() + b);
    DBuf<int64_t> d_member_at(member_at.size()), d_ref_start((size_t)n_ref + 1), d_win_off((size_t)n_ref + 1);
    DBuf<int32_t> d_ref(k), d_pos(k), d_end(k), d_max_end((size_t)n_ref);
    DBuf<uint64_t> d_vs(k), d_ve(k), d_bkey(k), d_ekey(k), d_M(k), d_first((size_t)n_ref), d_last((size_t)n_ref);
    d_member_at.upload(member_at.data(), member_at.size(), st); d_ref_start.upload(ref_start.data(), ref_start.size(), st);
    d_ref.upload(s.ref.data(), k, st); d_pos.upload(s.pos.data(), k, st); d_end.upload(s.end.data(), k, st);
    bam_index_rec_kernel<<<dim3(flat_grid(s.n)), dim3(256), 0, st>>>(s.d_perm.p, s.d_out_off.p, d_member_at.p, d_ref.p, d_pos.p, d_end.p, s.n, d_vs.p, d_ve.p, d_bkey.p, d_ekey.p);
    MM_KERNEL_CHECK();
    index_bins(s, d_bkey.p, d_vs.p, d_ve.p, st, &ckey, &cvs, &cve);
    inclusive_scan_max(s.tmp, d_ekey.p, d_M.p, k, st);
    bam_index_ref_kernel<<<dim3(flat_grid(n_ref)), dim3(256), 0, st>>>(d_ref_start.p, n_ref, d_M.p, d_vs.p, d_ve.p, d_max_end.p, d_first.p, d_last.p);
    MM_KERNEL_CHECK();
    const std::vector<int32_t> max_end = d_max_end.to_host(st);
    first_vs = d_first.to_host(st); last_ve = d_last.to_host(st);
    for (int32_t r = 0; r < n_ref; ++r) win_off[(size_t)r + 1] = win_off[(size_t)r] + mmbs::n_intervals(max_end[(size_t)r]);
    const int64_t n_win = win_off[(size_t)n_ref];
    DBuf<uint64_t> d_ioff((size_t)std::max<int64_t>(n_win, 1));
    d_win_off.upload(win_off.data(), win_off.size(), st);
    bam_index_linear_kernel<<<dim3(flat_grid(n_win)), dim3(256), 0, st>>>(d_ref_start.p, d_win_off.p, n_ref, d_M.p, d_vs.p, d_ioff.p);
    MM_KERNEL_CHECK();
    ioff = d_ioff.to_host(st, (size_t)n_win);
  }
  s.product = mmbs::bai_bytes(mmbs::BaiParts{n_ref, ref_start.data(), first_vs.data(), last_ve.data(), (int64_t)ckey.size(), ckey.data(), cvs.data(), cve.data(), win_off.data(), ioff.data()});
}

}  // namespace mm
