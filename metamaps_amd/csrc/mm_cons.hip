// The consensus of a group of contigs on the device (mm_consensus; mapDirectly --consensus; DESIGN.md section 1, "Consensus"; the definition: mm_cons_core.hpp,
// the text the host test runs).  The group's contigs lie behind one another: position p of contig c is g = gbase[c - contig_lo] + p, and every per-position
// array has one entry per g, so a call's memory is bounded by the group's bases.
//   candidates  mm_keytable.hip's finish_kept with min_count 1 and F: the intervals sorted, a row's depth from two binary searches, the kept rows compacted;
//               the payload keeps (w0, w1, depth) of a kept row on the device.  A kept row with depth < D stays in the list and is no candidate: rows at one
//               position share their depth, so the neighbour compares below never pair a candidate with such a row.
//   select      cons_endkey_kernel and an exclusive prefix maximum (rocPRIM) give every row the largest footprint end of the candidate deletions before it;
//               cons_del_kernel decides the deletions and clears their footprints in the positions' state (a lane its own run of up to 64, the wavefront a
//               longer one); cons_point_kernel then decides SNVs and insertions from the state at their position and the row before them, and stores the
//               alt in the state and the insertion's row in `ins`.
//   positions   cons_depth_kernel: two 32-bit atomics per interval into a difference array, then ONE flat inclusive scan: every contig's differences sum to
//               zero, so no segment flags.  cons_called_kernel counts the called positions.
//   offsets     cons_len_kernel: a position's output length; an exclusive scan; cons_lines_kernel: a contig's length and lines; a scan over the contigs.
//   emit        cons_emit_kernel: one thread per position writes its base, its insertion of up to 64 bases and the \n behind the column that ends a line or
//               the contig; the wavefront writes a longer insertion.  Neighbouring lanes write neighbouring bytes.  Reference bytes come through EditSeq::byte.
// Counters are summed per wavefront where its lanes share a contig and added with one 64-bit atomic each.  No kernel here waits for another workgroup; every
// loop runs over a length the host has checked (mmv::key_valid, the intervals' bounds) or over the steps of a binary search.
#include "mm_cons.hpp"
#include "mm_cons_core.hpp"
#include "mm_prims.hpp"
#include <string>

namespace mm {

namespace {
struct ConsLanes {                                                // the wavefronts of a 256-thread workgroup
  static constexpr uint32_t W = 64;
  __device__ uint32_t lane() const { return threadIdx.x & 63u; }
  __device__ uint64_t ballot(bool b) const { return (uint64_t)__ballot(b); }
  __device__ int64_t pick(int64_t v, uint32_t l) const { return (int64_t)__shfl((long long)v, (int)l, 64); }
};
// the group on the device: ng contigs from contig `lo` of the reference on, gbase[ng + 1]; need[c]: the called positions that make contig c written
struct ConsGroup { int64_t lo, ng, G; const uint64_t* gbase; const int64_t* need; };
__device__ __forceinline__ int64_t contig_of(const ConsGroup& g, int64_t at) { return mmp::bound(g.gbase, g.ng + 1, (uint64_t)at, true) - 1; }

// v[k] to counter slot[k] of contig c (of the group) for the lanes that are `in`; reached by every lane of a wavefront.  Rows and positions lie in contig
// order: a wavefront whose lanes share a contig (nearly every one) adds its sums once, integer sums in any order.
template <int K> __device__ __forceinline__ void cons_add(unsigned long long* __restrict__ stats, int64_t c, bool in, const int (&slot)[K], const unsigned long long (&v)[K]) {
  const uint64_t active = (uint64_t)__ballot(in);
  if (!active) return;
  const int lead = __ffsll((long long)active) - 1;
  const int64_t c0 = (int64_t)__shfl((long long)c, lead, 64);
  if (__all(!in || c == c0)) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      unsigned long long x = in ? v[k] : 0;
      for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
      if ((int)(threadIdx.x & 63) == lead && x) atomicAdd(&stats[c0 * mmc::STATS + slot[k]], x);
    }
  } else if (in) {
#pragma unroll
    for (int k = 0; k < K; ++k) if (v[k]) atomicAdd(&stats[c * mmc::STATS + slot[k]], v[k]);
  }
}
}  // namespace

// the intervals sorted by start key (end_of[i] belongs to starts[i]): +1 at the first base, -1 behind the last; diff has G + 1 entries
__global__ void __launch_bounds__(256) cons_depth_kernel(const uint64_t* __restrict__ starts, const uint64_t* __restrict__ end_of, int64_t n_iv, ConsGroup g, int32_t* __restrict__ diff,
                                                         unsigned long long* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = i < n_iv;
  const int64_t c = in ? (int64_t)(starts[i] >> 32) - g.lo : 0;
  if (in) {
    atomicAdd(&diff[g.gbase[c] + (starts[i] & 0xFFFFFFFFull)], 1);
    atomicAdd(&diff[g.gbase[c] + (end_of[i] & 0xFFFFFFFFull) + 1], -1);
  }
  cons_add<1>(stats, c, in, {mmc::ALIGNMENTS}, {1ull});
}
struct ConsRows { int64_t n; const uint64_t* w0; const uint64_t* w1; const uint32_t* depth; };   // the kept rows in key order
__global__ void __launch_bounds__(256) cons_endkey_kernel(ConsRows r, int64_t min_depth, uint64_t* __restrict__ endkey) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < r.n) endkey[i] = (int64_t)r.depth[i] >= min_depth ? mmc::del_end_key(r.w0[i], r.w1[i]) : 0;
}
// ends_before[i]: the exclusive prefix maximum of the end keys
__global__ void __launch_bounds__(256) cons_del_kernel(ConsRows r, int64_t min_depth, const uint64_t* __restrict__ ends_before, ConsGroup g, uint8_t* __restrict__ state,
                                                       unsigned long long* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool cand = i < r.n && mmc::is_del(r.w0[i]) && (int64_t)r.depth[i] >= min_depth;
  const uint64_t w0 = cand ? r.w0[i] : 0;
  const int64_t c = cand ? mmp::key_contig(w0) - g.lo : 0, n = cand ? (int64_t)r.w1[i] : 0;
  const bool applied = cand && mmc::del_applied(w0, ends_before[i]);
  ConsLanes p;
  mmc::clear_footprint(p, state, applied ? (int64_t)g.gbase[c] + mmp::key_pos(w0) + 1 : 0, n, applied);
  cons_add<3>(stats, c, cand, {mmc::DELETIONS, mmc::DELETED_BASES, mmc::DROPPED}, {applied ? 1ull : 0ull, applied ? (unsigned long long)n : 0ull, applied ? 0ull : 1ull});
}
// after every footprint is cleared; ins[g]: 1 + the row of the insertion applied at g
__global__ void __launch_bounds__(256) cons_point_kernel(ConsRows r, int64_t min_depth, ConsGroup g, uint8_t* __restrict__ state, uint32_t* __restrict__ ins,
                                                         unsigned long long* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool cand = i < r.n && !mmc::is_del(r.w0[i]) && (int64_t)r.depth[i] >= min_depth;
  const uint64_t w0 = cand ? r.w0[i] : 0;
  const int64_t c = cand ? mmp::key_contig(w0) - g.lo : 0;
  bool applied = false, snv = false;
  int64_t n = 0;
  if (cand) {
    const int64_t at = (int64_t)g.gbase[c] + mmp::key_pos(w0);
    applied = mmc::point_applied(w0, i > 0, i > 0 ? r.w0[i - 1] : 0, state[at]);
    snv = mmc::is_snv(w0);
    if (applied && snv) state[at] = mmc::snv_state(w0);           // (the position's only writer: one SNV is applied there, and it is not removed)
    if (applied && !snv) { ins[at] = (uint32_t)i + 1; n = mmv::ins_len(r.w1[i]); }
  }
  cons_add<4>(stats, c, cand, {mmc::SNVS, mmc::INSERTIONS, mmc::INSERTED_BASES, mmc::DROPPED},
              {applied && snv ? 1ull : 0ull, applied && !snv ? 1ull : 0ull, (unsigned long long)n, applied ? 0ull : 1ull});
}
__global__ void __launch_bounds__(256) cons_called_kernel(const int32_t* __restrict__ depth, int64_t min_depth, ConsGroup g, unsigned long long* __restrict__ stats) {
  const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = at < g.G;
  const int64_t c = in ? contig_of(g, at) : 0;
  cons_add<1>(stats, c, in, {mmc::CALLED}, {in && depth[at] >= min_depth ? 1ull : 0ull});
}
// a position's output length; olen[G] = 0 for the scan's total
__global__ void __launch_bounds__(256) cons_len_kernel(const uint8_t* __restrict__ state, const uint32_t* __restrict__ ins, const uint64_t* __restrict__ w1, ConsGroup g,
                                                       const unsigned long long* __restrict__ stats, uint32_t* __restrict__ olen) {
  const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (at > g.G) return;
  if (at == g.G) { olen[at] = 0; return; }
  const int64_t c = contig_of(g, at);
  const bool written = (int64_t)stats[c * mmc::STATS + mmc::CALLED] >= g.need[c];
  olen[at] = (uint32_t)mmc::out_len(state[at], ins[at] ? mmv::ins_len(w1[ins[at] - 1]) : 0, written);
}
// per contig: whether it is written, its consensus length and its lines; lines[ng] = 0 for the scan's total
__global__ void __launch_bounds__(256) cons_lines_kernel(const int64_t* __restrict__ off, ConsGroup g, int64_t width, unsigned long long* __restrict__ stats, int64_t* __restrict__ lines) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c > g.ng) return;
  if (c == g.ng) { lines[c] = 0; return; }
  const int64_t len = off[g.gbase[c + 1]] - off[g.gbase[c]];
  stats[c * mmc::STATS + mmc::WRITTEN] = (int64_t)stats[c * mmc::STATS + mmc::CALLED] >= g.need[c] ? 1 : 0;
  stats[c * mmc::STATS + mmc::LENGTH] = (unsigned long long)len;
  lines[c] = mmc::text_lines(len, width);
}
// off: the exclusive sums of olen; line_off: those of lines.  Contig c's text starts at off[gbase[c]] + line_off[c].
__global__ void __launch_bounds__(256) cons_emit_kernel(const uint8_t* __restrict__ state, const uint32_t* __restrict__ ins, const uint64_t* __restrict__ w1,
                                                        const int32_t* __restrict__ depth, int64_t min_depth, const int64_t* __restrict__ off, const int64_t* __restrict__ line_off,
                                                        ConsGroup g, int64_t width, EditSeq R, const uint64_t* __restrict__ r_base, uint8_t* __restrict__ text) {
  const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = at < g.G && off[at + 1] > off[at];
  int64_t o = 0, len = 0;
  uint8_t* mine = text;
  uint8_t base = 0;
  uint64_t iw = 0;
  if (live) {
    const int64_t c = contig_of(g, at), c_off = off[g.gbase[c]];
    o = off[at] - c_off; len = off[g.gbase[c + 1]] - c_off; mine = text + c_off + line_off[c];
    const uint8_t s = state[at];
    const bool from_ref = !(s >> 1) && depth[at] >= min_depth;    // (the reference's byte is read only where it is written)
    base = mmc::out_base(s, depth[at], min_depth, from_ref ? R.byte((int64_t)r_base[g.lo + c] + (at - (int64_t)g.gbase[c])) : (uint8_t)0);
    if (ins[at]) iw = w1[ins[at] - 1];
  }
  ConsLanes p;
  mmc::emit_position(p, mine, len, width, o, live, base, iw);
}

namespace {
struct ConsKeep {                                                 // a kept row's payload: its words and its depth stay on the device
  const uint64_t* w0; const uint64_t* w1; const uint32_t* depth; uint64_t* o0; uint64_t* o1; uint32_t* odepth;
  __device__ void operator()(int64_t i, int64_t o, int64_t, int64_t) const { o0[o] = w0[i]; o1[o] = w1[i]; odepth[o] = depth[i]; }
};
}  // namespace

void consensus_run(mm_ctx* ctx, const mm_seqset* ref, const ConsIn& cin, ConsResult* out) {
  const FinishIn& in = cin.table;
  hipStream_t st = ctx->stream;
  const bool timing = getenv("MM_CONS_TIMING") != nullptr;
  StageClock<3> clk(timing, st);                                   // intervals (upload and sorts), candidates
  StageClock<4> clk2(timing, st);                                  // select, positions, offsets, emit (with the text's way to the host)
  const int64_t nc = ref->count(), lo = cin.contig_lo, hi = cin.contig_hi;
  MM_REQUIRE(mmc::thresholds_ok(cin.min_depth, in.min_frac, cin.min_called, cin.line_width), MM_ERR_ARG,
             "mm_consensus: min_depth < 1, min_frac outside [0.5, 1], min_called outside [0, 1] or line_width < 1");
  MM_REQUIRE(0 <= lo && lo <= hi && hi <= nc, MM_ERR_ARG, "mm_consensus: [contig_lo, contig_hi) is no range of the reference's contigs");
  MM_REQUIRE(in.n_iv < ((int64_t)1 << 31), MM_ERR_LIMIT, "mm_consensus: 2^31 intervals or more (a position's depth is a 32-bit sum)");
  auto check_keys = [&] {                                         // before anything is launched: every later index is inside its array
    for (int64_t i = 0; i < in.n; ++i) {
      const uint64_t a = in.w0[i], b = in.w1[i];
      MM_REQUIRE(i == 0 || in.w0[i - 1] < a || (in.w0[i - 1] == a && in.w1[i - 1] < b), MM_ERR_ARG,
                 "mm_consensus: the keys are not ascending and unique (entry " + std::to_string(i) + "): pass a merged table");
      MM_REQUIRE(mmp::key_contig(a) < nc && mmv::key_valid(a, b, ref->len[(size_t)mmp::key_contig(a)]), MM_ERR_ARG,
                 "mm_consensus: entry " + std::to_string(i) + " names no position of the reference, or no allele");
      MM_REQUIRE(mmp::key_contig(a) >= lo && mmp::key_contig(a) < hi, MM_ERR_ARG, "mm_consensus: entry " + std::to_string(i) + " lies outside [contig_lo, contig_hi)");
    }
    for (int64_t i = 0; i < in.n_iv; ++i)
      MM_REQUIRE(in.iv_contig[i] >= lo && in.iv_contig[i] < hi, MM_ERR_ARG, "mm_consensus: interval " + std::to_string(i) + " lies outside [contig_lo, contig_hi)");
  };
  DBuf<uint64_t> d_w1, c_w0, c_w1; DBuf<uint32_t> c_depth;
  auto compact = [&](const KeptDev& rows) {
    const size_t k = (size_t)rows.n;
    d_w1.alloc(k); c_w0.alloc(k); c_w1.alloc(k); c_depth.alloc(k);
    d_w1.upload(in.w1, k, st);
    compact_kept(rows, ConsKeep{rows.w0, d_w1.p, rows.depth, c_w0.p, c_w1.p, c_depth.p}, st);
  };
  *out = ConsResult{};
  out->text_off.assign(1, 0);
  SortedIntervals iv;
  KeptRows kept;
  if (!finish_kept(ctx, ref, FinishIn{in.n, in.w0, in.w1, in.counts, in.n_iv, in.iv_contig, in.iv_first, in.iv_last, 1, in.min_frac}, "mm_consensus", check_keys, compact, clk, &iv, &kept))
    return;
  clk.stop(1);
  if (in.n_iv == 0) return;                                        // no contig has an interval: nothing is reported
  const int64_t nk = (int64_t)kept.w0.size(), ng = hi - lo;
  const ConsRows rows{nk, c_w0.p, c_w1.p, c_depth.p};

  std::vector<uint64_t> gbase((size_t)ng + 1, 0); std::vector<int64_t> need((size_t)ng);
  for (int64_t c = 0; c < ng; ++c) {
    gbase[(size_t)c + 1] = gbase[(size_t)c] + (uint64_t)ref->len[(size_t)(lo + c)];
    need[(size_t)c] = mmc::called_needed(cin.min_called, ref->len[(size_t)(lo + c)]);
  }
  const int64_t G = (int64_t)gbase[(size_t)ng];
  const size_t gs = (size_t)G;
  DBuf<uint64_t> d_gbase((size_t)ng + 1); DBuf<int64_t> d_need((size_t)ng);
  d_gbase.upload(gbase.data(), (size_t)ng + 1, st); d_need.upload(need.data(), (size_t)ng, st);
  const ConsGroup g{lo, ng, G, d_gbase.p, d_need.p};
  DBuf<uint8_t> tmp, d_state(gs); DBuf<uint32_t> d_ins(gs); DBuf<int32_t> d_depth(gs + 1); DBuf<unsigned long long> d_stats((size_t)ng * mmc::STATS);
  d_state.zero(st); d_ins.zero(st); d_depth.zero(st); d_stats.zero(st);

  clk2.start();
  if (nk) {
    DBuf<uint64_t> d_endkey((size_t)nk), d_before((size_t)nk);
    cons_endkey_kernel<<<dim3(flat_grid(nk)), dim3(256), 0, st>>>(rows, cin.min_depth, d_endkey.p); MM_KERNEL_CHECK();
    with_scratch(tmp, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, d_endkey.p, d_before.p, (uint64_t)0, (size_t)nk, rocprim::maximum<uint64_t>(), st); });
    cons_del_kernel<<<dim3(flat_grid(nk)), dim3(256), 0, st>>>(rows, cin.min_depth, d_before.p, g, d_state.p, d_stats.p); MM_KERNEL_CHECK();
    cons_point_kernel<<<dim3(flat_grid(nk)), dim3(256), 0, st>>>(rows, cin.min_depth, g, d_state.p, d_ins.p, d_stats.p); MM_KERNEL_CHECK();
    MM_HIP(mm::stream_sync(st));                                   // (the buffers of this scope)
  }
  clk2.stop(0);

  clk2.start();
  cons_depth_kernel<<<dim3(flat_grid(in.n_iv)), dim3(256), 0, st>>>(iv.starts.p, iv.end_of.p, in.n_iv, g, d_depth.p, d_stats.p); MM_KERNEL_CHECK();
  with_scratch(tmp, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, d_depth.p, d_depth.p, gs + 1, rocprim::plus<int32_t>(), st); });
  cons_called_kernel<<<dim3(flat_grid(G)), dim3(256), 0, st>>>(d_depth.p, cin.min_depth, g, d_stats.p); MM_KERNEL_CHECK();
  clk2.stop(1);

  clk2.start();
  DBuf<uint32_t> d_olen(gs + 1); DBuf<int64_t> d_off(gs + 1), d_lines((size_t)ng + 1), d_line_off((size_t)ng + 1);
  cons_len_kernel<<<dim3(flat_grid(G + 1)), dim3(256), 0, st>>>(d_state.p, d_ins.p, c_w1.p, g, d_stats.p, d_olen.p); MM_KERNEL_CHECK();
  exclusive_scan(tmp, d_olen.p, d_off.p, gs + 1, st);
  cons_lines_kernel<<<dim3(flat_grid(ng + 1)), dim3(256), 0, st>>>(d_off.p, g, cin.line_width, d_stats.p, d_lines.p); MM_KERNEL_CHECK();
  exclusive_scan(tmp, d_lines.p, d_line_off.p, (size_t)ng + 1, st);
  int64_t bases = 0, lines = 0;
  d_off.download(&bases, 1, st, gs); d_line_off.download(&lines, 1, st, (size_t)ng);
  const std::vector<unsigned long long> stats = d_stats.to_host(st);
  d_olen.release();
  clk2.stop(2);

  clk2.start();
  const size_t bytes = (size_t)(bases + lines);
  if (bytes) {
    DBuf<uint8_t> d_text(bytes);
    cons_emit_kernel<<<dim3(flat_grid(G)), dim3(256), 0, st>>>(d_state.p, d_ins.p, c_w1.p, d_depth.p, cin.min_depth, d_off.p, d_line_off.p, g, cin.line_width, edit_seq(ref), ref->d_base.p,
                                                               d_text.p); MM_KERNEL_CHECK();
    out->text = d_text.to_host(st);
  }
  clk2.stop(3);

  for (int64_t c = 0; c < ng; ++c) {
    const unsigned long long* s = &stats[(size_t)c * mmc::STATS];
    if (!s[mmc::ALIGNMENTS]) continue;
    out->contig.push_back((int32_t)(lo + c));
    for (int k = 0; k < mmc::STATS; ++k) out->stats.push_back((int64_t)s[k]);
    if (!s[mmc::WRITTEN]) continue;
    out->written.push_back((int32_t)(lo + c));
    out->text_off.push_back(out->text_off.back() + mmc::text_bytes((int64_t)s[mmc::LENGTH], cin.line_width));
  }
  MM_REQUIRE((size_t)out->text_off.back() == bytes, MM_ERR_DEVICE, "mm_consensus: the contigs' texts do not add up to the bytes written");
  if (timing)
    fprintf(stderr, "MM_CONS_TIMING consensus: intervals %.3f candidates %.3f select %.3f positions %.3f offsets %.3f emit %.3f ms; contigs [%lld, %lld), %lld bases, %lld entries, "
            "%lld intervals, %lld kept, %zu contigs written, %zu B of text\n", clk.ms[0], clk.ms[1], clk2.ms[0], clk2.ms[1], clk2.ms[2], clk2.ms[3], (long long)lo, (long long)hi, (long long)G,
            (long long)in.n, (long long)in.n_iv, (long long)nk, out->written.size(), bytes);
}

}  // namespace mm
