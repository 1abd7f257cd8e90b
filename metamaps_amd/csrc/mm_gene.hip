// Gene-level analysis of the reads' best mappings (classify --genes; the reference does it in geneLevelAnalysis.pl; DESIGN.md section 4,
// "Gene-level analysis"): an interval join of the mappings against the annotated genes of their contigs, per gene group the number of
// overlapping mappings and the median of their identities, per annotation feature the number of mappings that overlap a gene carrying it.
//   walk      gene_walk_kernel runs mm_gene_core.hpp's gene_stab for every mapping of a range: a lane per mapping, and the whole wavefront,
//             one mapping after the other, for the mappings of its 64 with more than GENE_LANE_SPAN candidates (a 200 kb read, a gene-dense
//             contig).  What a walk does with the genes it finds is its Op: count (a), fill (c), median keys (d).  The reports of a mapping
//             come in descending gene index in either shape, so the split point changes no result.
//   (a)       overlaps per mapping, and feature ids behind them     (b) rocprim::exclusive_scan of both
//   (c)       (mapping, group) pairs at their offsets; reads per group with 64-bit vector atomics
//   (e)       every pair expands to keys feature << mb | mapping through group_feat_off; the keys are radix-sorted; heads of runs of equal
//             keys are counted per feature (a mapping counts once per feature however many of its genes carry it)
//   (d)       identities get ranks from one sort of their bit patterns (mm_prims.hpp, rank_by_bits; non-negative doubles order as their 64-bit patterns); a second walk
//             writes the keys group << rb | rank into the group's range [first[g], first[g] + n_g) (first: the scan of the reads per group;
//             the place inside the range comes from a cursor, the sort that follows makes it immaterial); the keys are radix-sorted; the
//             median of group g is the identity whose rank sits at first[g] + (n_g - 1) / 2
// Tiling: (c) and (e) run over ranges of mappings that hold at most `budget` pairs and `budget` feature keys (a single mapping beyond it is a
// range of its own), group and feature counts add up; (d) runs over ranges of groups that hold at most `budget` keys, each with a walk over
// all mappings that keeps the range's groups — a group's selection is never split.  No result depends on the budget.
// The sorts and scans are rocprim's, through mm_prims.hpp, and share the job's one scratch buffer.  All pair, key and mapping indices are 64-bit; positions are int32.
#include "mm_gene.hpp"
#include "mm_prims.hpp"
#include <algorithm>
#include <cmath>
#include <limits>

namespace mm {

struct GeneMapsDev { const int32_t* contig; const int32_t* s; const int32_t* e; };

struct GeneWave {                                                 // the 64 lanes of a wavefront share a mapping
  __device__ int lane() const { return (int)(threadIdx.x & 63); }
  __device__ int width() const { return 64; }
  __device__ int place(bool hit, int* total) const {
    const unsigned long long m = __ballot(hit);
    *total = __popcll(m);
    return __popcll(m & ((1ull << lane()) - 1));
  }
};
__device__ inline int64_t gene_wave_sum(int64_t x) { for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64); return x; }

// (a) cnt[m], kcnt[m]
struct GeneCountOp {
  const int32_t* group; const int64_t* foff; uint64_t* cnt; uint64_t* kcnt;
  using Visit = GeneCount;
  __device__ Visit begin(int64_t) const { return GeneCount{group, foff}; }
  __device__ void end_lane(int64_t m, const Visit& v) const { cnt[m] = (uint64_t)v.n; kcnt[m] = (uint64_t)v.nk; }
  __device__ void end_wave(int64_t m, const Visit& v) const {
    const int64_t n = gene_wave_sum(v.n), nk = gene_wave_sum(v.nk);
    if ((threadIdx.x & 63) == 0) { cnt[m] = (uint64_t)n; kcnt[m] = (uint64_t)nk; }
  }
};
// (c) the pairs of the mappings of a tile, from pair_off[m] - p0 on; reads per group
struct GeneFillOp {
  const int32_t* group; const uint64_t* pair_off; uint64_t p0; int64_t* pair_map; int32_t* pair_group; unsigned long long* group_reads;
  struct Visit {
    const GeneFillOp* o; int64_t m, at;
    template <class G> __device__ void operator()(const G& g, int64_t j, bool hit) {
      int total; const int k = g.place(hit, &total);
      if (hit) { const int32_t gr = o->group[j]; o->pair_map[at + k] = m; o->pair_group[at + k] = gr; atomicAdd(&o->group_reads[gr], 1ull); }
      at += total;
    }
  };
  __device__ Visit begin(int64_t m) const { return Visit{this, m, (int64_t)(pair_off[m] - p0)}; }
  __device__ void end_lane(int64_t, const Visit&) const {}
  __device__ void end_wave(int64_t, const Visit&) const {}
};
// (d) the median keys of the groups [g0, g1)
struct GeneMedianOp {
  const int32_t* group; int32_t g0, g1; const uint64_t* first; uint64_t f0; unsigned long long* cursor; const uint32_t* rank; int rb; uint64_t* keys;
  struct Visit {
    const GeneMedianOp* o; int64_t m;
    template <class G> __device__ void operator()(const G&, int64_t j, bool hit) {
      if (!hit) return;
      const int32_t gr = o->group[j];
      if (gr < o->g0 || gr >= o->g1) return;
      const uint64_t slot = o->first[gr] - o->f0 + atomicAdd(&o->cursor[gr], 1ull);
      o->keys[slot] = (uint64_t)(gr - o->g0) << o->rb | o->rank[m];
    }
  };
  __device__ Visit begin(int64_t m) const { return Visit{this, m}; }
  __device__ void end_lane(int64_t, const Visit&) const {}
  __device__ void end_wave(int64_t, const Visit&) const {}
};

// the mappings [m0, m1): every wavefront takes 64 consecutive ones at a time
template <class Op> __global__ void __launch_bounds__(256) gene_walk_kernel(GeneTable T, GeneMapsDev M, int64_t m0, int64_t m1, Op op) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * 4, wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  for (int64_t base = m0 + wave * 64; base < m1; base += n_waves * 64) {   // (the same for every lane of the wavefront)
    const int64_t m = base + lane;
    int64_t lo = 0, hi = 0; int32_t s = 0;
    if (m < m1) { s = M.s[m]; gene_span(T, M.contig[m], s, M.e[m], &lo, &hi); }
    const bool wide = hi - lo > GENE_LANE_SPAN;
    if (m < m1 && !wide) {
      typename Op::Visit v = op.begin(m);
      gene_stab(GeneSerial{}, T, lo, hi, s, v);
      op.end_lane(m, v);
    }
    for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1) {   // the wide ones, by all 64 lanes
      const int src = __ffsll(todo) - 1;
      const int64_t wlo = __shfl(lo, src, 64), whi = __shfl(hi, src, 64);
      const int32_t ws = __shfl(s, src, 64);
      typename Op::Visit v = op.begin(base + src);
      gene_stab(GeneWave{}, T, wlo, whi, ws, v);
      op.end_wave(base + src, v);
    }
  }
}

__global__ void __launch_bounds__(256) gene_rank_kernel(const uint32_t* __restrict__ perm, int64_t n, uint32_t* __restrict__ rank) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) rank[perm[i]] = (uint32_t)i;
}
// (e) feature ids per pair (nf[n] = 0 for the scan's total), then the keys
__global__ void __launch_bounds__(256) gene_pair_feats_kernel(const int32_t* __restrict__ pair_group, int64_t n, const int64_t* __restrict__ foff, uint64_t* __restrict__ nf) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) nf[k] = (uint64_t)(foff[pair_group[k] + 1] - foff[pair_group[k]]);
  else if (k == n) nf[k] = 0;
}
__global__ void __launch_bounds__(256) gene_expand_kernel(const int64_t* __restrict__ pair_map, const int32_t* __restrict__ pair_group, int64_t n, int64_t m0,
                                                          const int64_t* __restrict__ foff, const int32_t* __restrict__ feat, const uint64_t* __restrict__ koff, int mb,
                                                          uint64_t* __restrict__ keys) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int64_t a = foff[pair_group[k]], b = foff[pair_group[k] + 1];
  const uint64_t ml = (uint64_t)(pair_map[k] - m0);
  uint64_t at = koff[k];
  for (int64_t i = a; i < b; ++i) keys[at++] = (uint64_t)feat[i] << mb | ml;
}
// heads of runs of equal keys, per feature: a thread walks GENE_HEAD_ITEMS sorted keys and adds once per feature it meets
constexpr int GENE_HEAD_ITEMS = 16;
__global__ void __launch_bounds__(256) gene_heads_kernel(const uint64_t* __restrict__ keys, int64_t n, int mb, unsigned long long* __restrict__ feat_reads) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * GENE_HEAD_ITEMS, i1 = min(i0 + GENE_HEAD_ITEMS, n);
  uint64_t cur = 0, run = 0;
  for (int64_t i = i0; i < i1; ++i) {
    const uint64_t key = keys[i], f = key >> mb;
    if (f != cur) { if (run) atomicAdd(&feat_reads[cur], (unsigned long long)run); cur = f; run = 0; }
    if (i == 0 || keys[i - 1] != key) ++run;
  }
  if (run) atomicAdd(&feat_reads[cur], (unsigned long long)run);
}
__global__ void __launch_bounds__(256) gene_select_kernel(int32_t g0, int32_t g1, const unsigned long long* __restrict__ group_reads, const uint64_t* __restrict__ first,
                                                          uint64_t f0, const uint64_t* __restrict__ keys, int rb, const uint64_t* __restrict__ ident_sorted,
                                                          uint64_t* __restrict__ median_bits) {
  const int64_t g = (int64_t)g0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= g1) return;
  const uint64_t n = group_reads[g];
  uint64_t bits = 0x7ff8000000000000ull;                          // NaN
  if (n) bits = ident_sorted[keys[first[g] - f0 + (n - 1) / 2] & ((1ull << rb) - 1)];
  median_bits[g] = bits;
}

namespace {

unsigned walk_grid(int64_t n) { return (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(n, 256), 1), 2048); }
struct GeneJob {
  const GeneIn& in; hipStream_t st; int64_t budget;
  StageClock<6> clk;                                               // MM_GENE_TIMING=1: ranks, count, scan, fill, features, medians on stderr
  int64_t NG = 0, NM = 0; int rb = 1;
  DBuf<int64_t> d_off, d_foff; DBuf<int32_t> d_start, d_stop, d_pmax, d_group, d_feat, d_mc, d_ms, d_me;
  DBuf<uint32_t> d_rank; DBuf<uint64_t> d_ident_sorted, d_cnt, d_kcnt, d_pair_off, d_key_off, d_first;
  DBuf<unsigned long long> d_group_reads, d_feat_reads, d_cursor;
  DBuf<uint8_t> tmp;
  std::vector<uint64_t> h_pair_off, h_key_off;
  GeneTable T{}; GeneMapsDev M{};

  GeneJob(const GeneIn& in_, hipStream_t st_, int64_t budget_) : in(in_), st(st_), budget(budget_), clk(getenv("MM_GENE_TIMING") != nullptr, st_) {}

  void report(size_t map_tiles, size_t group_tiles) const {
    if (clk.on) fprintf(stderr, "MM_GENE_TIMING ranks %.3f count %.3f scan %.3f fill %.3f features %.3f medians %.3f ms; %lld pairs, %lld feature keys, %zu mapping tiles, %zu group tiles\n",
                        clk.ms[0], clk.ms[1], clk.ms[2], clk.ms[3], clk.ms[4], clk.ms[5], (long long)h_pair_off[(size_t)NM], (long long)h_key_off[(size_t)NM], map_tiles, group_tiles);
  }
  void upload() {
    NG = in.contig_gene_off[in.n_contigs]; NM = in.n_maps;
    const size_t ng = (size_t)NG, nm = (size_t)NM, nc = (size_t)in.n_contigs, ngr = (size_t)in.n_groups, nfi = (size_t)in.group_feat_off[in.n_groups];
    std::vector<int32_t> pmax(ng);
    gene_prefix_max(in.n_contigs, in.contig_gene_off, in.gene_stop, pmax.data());
    d_off.alloc(nc + 1); d_off.upload(in.contig_gene_off, nc + 1, st);
    d_start.alloc(ng); d_start.upload(in.gene_start, ng, st);
    d_stop.alloc(ng); d_stop.upload(in.gene_stop, ng, st);
    d_pmax.alloc(ng); d_pmax.upload(pmax.data(), ng, st);
    d_group.alloc(ng); d_group.upload(in.gene_group, ng, st);
    d_foff.alloc(ngr + 1); d_foff.upload(in.group_feat_off, ngr + 1, st);
    d_feat.alloc(std::max<size_t>(nfi, 1)); d_feat.upload(in.group_feat, nfi, st);
    d_mc.alloc(nm); d_mc.upload(in.map_contig, nm, st);
    d_ms.alloc(nm); d_ms.upload(in.map_start, nm, st);
    d_me.alloc(nm); d_me.upload(in.map_stop, nm, st);
    d_group_reads.alloc(ngr); d_group_reads.zero(st);
    d_feat_reads.alloc(std::max<size_t>((size_t)in.n_feats, 1)); d_feat_reads.zero(st);
    MM_HIP(mm::stream_sync(st));                                   // (pmax goes out of scope)
    T = GeneTable{d_off.p, d_start.p, d_stop.p, d_pmax.p};
    M = GeneMapsDev{d_mc.p, d_ms.p, d_me.p};
  }
  // rank[m] of the identities in ascending order, and the identities in that order
  void ranks() {
    clk.start();
    const size_t nm = (size_t)NM;
    rb = bits_for((uint64_t)NM);
    std::vector<uint64_t> bits(nm);
    for (size_t m = 0; m < nm; ++m) { const double x = in.map_ident[m] + 0.0; memcpy(&bits[m], &x, 8); }   // (-0.0 + 0.0 is +0.0)
    DBuf<uint64_t> d_bits(nm); DBuf<uint32_t> d_iota(nm), d_perm(nm);
    d_bits.upload(bits.data(), nm, st);
    d_ident_sorted.alloc(nm); d_rank.alloc(nm);
    rank_by_bits(tmp, d_bits.p, d_ident_sorted.p, d_iota.p, d_perm.p, nm, st);
    gene_rank_kernel<<<dim3(flat_grid(NM)), dim3(256), 0, st>>>(d_perm.p, NM, d_rank.p); MM_KERNEL_CHECK();
    MM_HIP(mm::stream_sync(st));                                   // (bits, and the buffers of this scope)
    clk.stop(0);
  }
  // (a), (b): the offsets of every mapping's pairs and feature keys, on the device and on the host
  void count() {
    clk.start();
    const size_t nm = (size_t)NM;
    d_cnt.alloc(nm + 1); d_kcnt.alloc(nm + 1); d_pair_off.alloc(nm + 1); d_key_off.alloc(nm + 1);
    MM_HIP(hipMemsetAsync(d_cnt.p + nm, 0, 8, st)); MM_HIP(hipMemsetAsync(d_kcnt.p + nm, 0, 8, st));
    gene_walk_kernel<<<dim3(walk_grid(NM)), dim3(256), 0, st>>>(T, M, (int64_t)0, NM, GeneCountOp{d_group.p, in.n_feats > 0 ? d_foff.p : nullptr, d_cnt.p, d_kcnt.p});
    MM_KERNEL_CHECK();
    clk.stop(1);
    clk.start();
    exclusive_scan(tmp, d_cnt.p, d_pair_off.p, nm + 1, st); exclusive_scan(tmp, d_kcnt.p, d_key_off.p, nm + 1, st);
    h_pair_off = d_pair_off.to_host(st); h_key_off = d_key_off.to_host(st);
    clk.stop(2);
  }
  // (c), (e) for the mappings [m0, m1)
  void pairs_tile(int64_t m0, int64_t m1, bool features, DBuf<int64_t>& pair_map, DBuf<int32_t>& pair_group, DBuf<uint64_t>& nf, DBuf<uint64_t>& koff, DBuf<uint64_t>& keys, DBuf<uint64_t>& keys2) {
    const uint64_t p0 = h_pair_off[(size_t)m0];
    const int64_t np = (int64_t)(h_pair_off[(size_t)m1] - p0), nk = (int64_t)(h_key_off[(size_t)m1] - h_key_off[(size_t)m0]);
    if (np == 0) return;
    clk.start();
    gene_walk_kernel<<<dim3(walk_grid(m1 - m0)), dim3(256), 0, st>>>(T, M, m0, m1, GeneFillOp{d_group.p, d_pair_off.p, p0, pair_map.p, pair_group.p, d_group_reads.p});
    MM_KERNEL_CHECK();
    clk.stop(3);
    if (!features || nk == 0) return;
    clk.start();
    const int mb = bits_for((uint64_t)(m1 - m0));
    gene_pair_feats_kernel<<<dim3(flat_grid(np + 1)), dim3(256), 0, st>>>(pair_group.p, np, d_foff.p, nf.p); MM_KERNEL_CHECK();
    exclusive_scan(tmp, nf.p, koff.p, (size_t)np + 1, st);
    gene_expand_kernel<<<dim3(flat_grid(np)), dim3(256), 0, st>>>(pair_map.p, pair_group.p, np, m0, d_foff.p, d_feat.p, koff.p, mb, keys.p); MM_KERNEL_CHECK();
    sort_keys(tmp, keys.p, keys2.p, (size_t)nk, 0, mb + bits_for((uint64_t)in.n_feats), st);
    gene_heads_kernel<<<dim3(flat_grid(ceil_div(nk, GENE_HEAD_ITEMS))), dim3(256), 0, st>>>(keys2.p, nk, mb, d_feat_reads.p); MM_KERNEL_CHECK();
    clk.stop(4);
  }
  // ranges [cut[i], cut[i+1]) of 0..n whose sizes by every one of the ascending `offs` stay within the budget (a single item beyond it: a range of its own)
  std::vector<int64_t> cuts(int64_t n, std::initializer_list<const std::vector<uint64_t>*> offs) const {
    std::vector<int64_t> cut{0};
    while (cut.back() < n) {
      const int64_t a = cut.back();
      int64_t b = n;
      for (const auto* o : offs) b = std::min<int64_t>(b, (std::upper_bound(o->begin() + a, o->begin() + n + 1, (*o)[(size_t)a] + (uint64_t)budget) - o->begin()) - 1);
      cut.push_back(std::max(b, a + 1));
    }
    return cut;
  }
  size_t pairs_and_features(bool features) {
    const std::vector<int64_t> cut = cuts(NM, {&h_pair_off, &h_key_off});
    int64_t max_p = 0, max_k = 0;
    for (size_t i = 0; i + 1 < cut.size(); ++i) {
      max_p = std::max<int64_t>(max_p, (int64_t)(h_pair_off[(size_t)cut[i + 1]] - h_pair_off[(size_t)cut[i]]));
      max_k = std::max<int64_t>(max_k, (int64_t)(h_key_off[(size_t)cut[i + 1]] - h_key_off[(size_t)cut[i]]));
    }
    if (max_p == 0) return cut.size() - 1;
    const size_t kp = features && max_k > 0 ? (size_t)max_k : 0;
    DBuf<int64_t> pair_map((size_t)max_p); DBuf<int32_t> pair_group((size_t)max_p);
    DBuf<uint64_t> nf(kp ? (size_t)max_p + 1 : 0), koff(kp ? (size_t)max_p + 1 : 0), keys(kp), keys2(kp);
    for (size_t i = 0; i + 1 < cut.size(); ++i) pairs_tile(cut[i], cut[i + 1], kp > 0, pair_map, pair_group, nf, koff, keys, keys2);
    MM_HIP(mm::stream_sync(st));
    return cut.size() - 1;
  }
  // (d): group_reads is final; medians of all groups, range of groups after range
  size_t medians(const std::vector<unsigned long long>& h_reads, double* group_median) {
    clk.start();
    const size_t ngr = (size_t)in.n_groups;
    std::vector<uint64_t> h_first(ngr + 1, 0);
    for (size_t g = 0; g < ngr; ++g) h_first[g + 1] = h_first[g] + h_reads[g];
    d_first.alloc(ngr + 1); d_first.upload(h_first.data(), ngr + 1, st);
    d_cursor.alloc(ngr); d_cursor.zero(st);
    const std::vector<int64_t> cut = cuts(in.n_groups, {&h_first});
    uint64_t max_k = 0;
    for (size_t i = 0; i + 1 < cut.size(); ++i) max_k = std::max(max_k, h_first[(size_t)cut[i + 1]] - h_first[(size_t)cut[i]]);
    DBuf<uint64_t> keys((size_t)max_k), keys2((size_t)max_k), med(ngr);
    for (size_t i = 0; i + 1 < cut.size(); ++i) {
      const int32_t g0 = (int32_t)cut[i], g1 = (int32_t)cut[i + 1];
      const uint64_t f0 = h_first[(size_t)g0], nk = h_first[(size_t)g1] - f0;
      if (nk > 0) {
        gene_walk_kernel<<<dim3(walk_grid(NM)), dim3(256), 0, st>>>(T, M, (int64_t)0, NM, GeneMedianOp{d_group.p, g0, g1, d_first.p, f0, d_cursor.p, d_rank.p, rb, keys.p});
        MM_KERNEL_CHECK();
        sort_keys(tmp, keys.p, keys2.p, (size_t)nk, 0, rb + bits_for((uint64_t)(g1 - g0)), st);
      }
      gene_select_kernel<<<dim3(flat_grid(g1 - g0)), dim3(256), 0, st>>>(g0, g1, d_group_reads.p, d_first.p, f0, keys2.p, rb, d_ident_sorted.p, med.p); MM_KERNEL_CHECK();
    }
    static_assert(sizeof(double) == sizeof(uint64_t), "medians are copied as bit patterns");
    med.download((uint64_t*)group_median, ngr, st);
    MM_HIP(mm::stream_sync(st));
    clk.stop(5);
    return cut.size() - 1;
  }
};

int64_t gene_budget() {
  const char* e = getenv("MM_GENE_PAIR_BUDGET");
  return e && atoll(e) > 0 ? atoll(e) : GENE_PAIR_BUDGET;
}

}  // namespace

void gene_overlap_run(mm_ctx* ctx, const GeneIn& in, int64_t* group_reads, double* group_median, int64_t* feat_reads, int64_t* maps_on_annotated) {
  int bad = gene_table_check(in.n_contigs, in.contig_gene_off, in.gene_start, in.gene_stop, in.gene_group, in.n_groups, in.group_feat_off, in.group_feat, in.n_feats);
  if (!bad) bad = gene_maps_check(in.n_maps, in.map_contig, in.map_start, in.map_stop, in.map_ident, in.n_contigs);
  MM_REQUIRE(!bad, MM_ERR_ARG, std::string("mm_gene_overlap: ") + gene_arg_message(bad));
  MM_REQUIRE(in.n_maps < ((int64_t)1 << 32), MM_ERR_LIMIT, "mm_gene_overlap: 2^32 mappings or more in one call");
  const int64_t NG = in.contig_gene_off[in.n_contigs];
  std::fill(group_reads, group_reads + in.n_groups, (int64_t)0);
  std::fill(group_median, group_median + in.n_groups, std::numeric_limits<double>::quiet_NaN());
  if (feat_reads) std::fill(feat_reads, feat_reads + in.n_feats, (int64_t)0);
  if (maps_on_annotated) {
    int64_t n = 0;
    for (int64_t m = 0; m < in.n_maps; ++m) n += in.contig_gene_off[in.map_contig[m] + 1] > in.contig_gene_off[in.map_contig[m]];
    *maps_on_annotated = n;
  }
  if (NG == 0 || in.n_maps == 0) return;
  GeneJob J(in, ctx->stream, gene_budget());
  J.upload();
  J.ranks();
  J.count();
  const size_t map_tiles = J.pairs_and_features(feat_reads != nullptr && in.n_feats > 0);
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are copied as they lie");
  std::vector<unsigned long long> h_reads = J.d_group_reads.to_host(J.st, (size_t)in.n_groups);
  std::copy(h_reads.begin(), h_reads.end(), group_reads);
  if (feat_reads) { J.d_feat_reads.download((unsigned long long*)feat_reads, (size_t)in.n_feats, J.st); MM_HIP(mm::stream_sync(J.st)); }
  const size_t group_tiles = J.h_pair_off[(size_t)in.n_maps] > 0 ? J.medians(h_reads, group_median) : 0;
  J.report(map_tiles, group_tiles);
}

}  // namespace mm
