// Methylation per sequence motif on the device (mm_mod_motifs; mapDirectly --mod-motifs; DESIGN.md section 1, "Modification motifs"; the definition:
// mm_motif_core.hpp, the text the host test runs).
//   scan    motif_scan_kernel: a workgroup of 256 threads takes a tile of 2 048 consecutive stream positions.  It stages the tile and a halo of 32 positions
//           behind it in LDS as one-hot nibbles, 8 per word, straight from the packed 2-bit words (a thread expands 16 bits), and clears the nibbles of the
//           exception runs that touch the tile (EditSeq::narrowed once per workgroup, one atomic AND per word and run).  A thread owns 8 consecutive window
//           starts: 5 LDS words give it 160 bits, which it shifts by a nibble per start, cuts at its contig's end (the contigs are padded to 16 bases in
//           the stream, and a window never looks into the next one) and tests against every motif's two 128-bit masks with AND and popcount.  Occurrences
//           are counted by window start, so nothing is staged in front of the tile.  The counts are summed over the wavefront by butterflies and over the
//           workgroup in LDS where the whole tile lies in one contig, and added per (listed contig, motif) with 64-bit atomics; a tile of several contigs
//           adds per thread.  Tiles without a listed contig leave after the lookup.  Every LDS index is below 260 = SCAN_THREADS + 4 by construction.
//   sites   motif_rows_kernel, shaped as mod_rows_kernel: the head of every (contig, position, strand) segment of the group's table slice runs
//           mmt::site_rows (count pass: the covered rows counted, their sums added with atomics; emit pass behind a scan: the rows written).  Under combined
//           strands the rows are then put into the units' order by two stable radix sorts of their indices.
// No kernel waits for another workgroup.
#include "mm_motif.hpp"
#include "mm_edit_seq.hpp"
#include "mm_mods.hpp"
#include "mm_prims.hpp"

namespace mm {

namespace {
constexpr int T = mmt::SCAN_THREADS, PER = mmt::SCAN_PER_THREAD, TILE = mmt::SCAN_TILE, WORDS = T + 4;
static_assert(PER == 8 && TILE == T * PER && mmt::HALO < 32, "a thread's starts are the nibbles of one staged word; the halo is four words");

// 8 two-bit codes (16 bits) as 8 one-hot nibbles
__device__ uint32_t nibbles_of(uint32_t bits) {
  uint32_t w = 0;
  for (int k = 0; k < 8; ++k) w |= 1u << (4 * k + ((bits >> (2 * k)) & 3u));
  return w;
}

// sites[rank * M.n + j]: the occurrences of motif j (both orientations; the + ones alone under combine) that start in the listed contig of that rank.
// rank[c - lo]: the rank of contig c of [lo, hi) among the listed ones, -1 for the others.  Tile blockIdx.x + tile0 of the stream.
__global__ void __launch_bounds__(T) motif_scan_kernel(const uint32_t* __restrict__ packed, int64_t n_words, EditSeq R, const uint64_t* __restrict__ r_base, const int32_t* __restrict__ r_len,
                                                       int32_t lo, int32_t hi, const int32_t* __restrict__ rank, mmt::Motifs M, int32_t combine, int64_t tile0,
                                                       unsigned long long* __restrict__ sites) {
  __shared__ uint32_t nib[WORDS];
  __shared__ unsigned long long acc[mmt::MAX_MOTIFS];
  __shared__ int64_t sh_run0, sh_runs;
  __shared__ int sh_any, sh_rank, sh_mixed;
  const int t = (int)threadIdx.x;
  const int64_t t0 = (tile0 + (int64_t)blockIdx.x) * TILE, s0 = t0 + (int64_t)t * PER;
  if (t == 0) { sh_any = 0; sh_rank = -1; sh_mixed = 0; }
  if (t < mmt::MAX_MOTIFS) acc[t] = 0;
  // the last contig of [lo, hi) that starts at or before s0 (lo where none does)
  int32_t c0 = lo;
  for (int32_t a = lo + 1, b = hi; a < b;) { const int32_t mid = a + (b - a) / 2; if (r_base[mid] <= (uint64_t)s0) { c0 = mid; a = mid + 1; } else b = mid; }
  bool any = false;
  for (int32_t c = c0; c < hi && r_base[c] < (uint64_t)(s0 + PER); ++c)
    if (rank[c - lo] >= 0 && (uint64_t)s0 < r_base[c] + (uint64_t)r_len[c]) any = true;
  __syncthreads();
  if (any) sh_any = 1;
  __syncthreads();
  if (!sh_any) return;                                             // (the same in every thread)

  for (int w = t; w < WORDS; w += T) {
    const int64_t p = t0 + (int64_t)w * 8, word = p >> 4;
    nib[w] = word < n_words ? nibbles_of(packed[word] >> (2 * (p & 15)) & 0xFFFFu) : 0u;
  }
  if (t == 0) {
    const EditSeq N = R.narrowed((uint64_t)t0, (uint64_t)t0 + TILE + 32);
    sh_run0 = N.exc_start - R.exc_start; sh_runs = N.n_exc;
  }
  __syncthreads();
  for (int64_t r = sh_run0 + t; r < sh_run0 + sh_runs; r += T) {   // the runs that touch [t0, t0 + TILE + 32), cut to it
    const int64_t a = std::max<int64_t>((int64_t)R.exc_start[r], t0) - t0, b = std::min<int64_t>((int64_t)(R.exc_start[r] + R.exc_len[r]), t0 + TILE + 32) - t0;
    for (int64_t w = a >> 3; w * 8 < b; ++w) {                     // (a >= 0, b <= 8 * WORDS: w in [0, WORDS))
      uint32_t clear = 0;
      for (int k = 0; k < 8; ++k) if (w * 8 + k >= a && w * 8 + k < b) clear |= 0xFu << (4 * k);
      atomicAnd(&nib[w], ~clear);
    }
  }
  __syncthreads();

  const uint64_t w0 = (uint64_t)nib[t] | (uint64_t)nib[t + 1] << 32, w1 = (uint64_t)nib[t + 2] | (uint64_t)nib[t + 3] << 32, w2 = nib[t + 4];
  uint32_t cnt[mmt::MAX_MOTIFS] = {0, 0, 0, 0, 0, 0, 0, 0};
  int32_t c = c0, mine = -1;                                       // mine: the rank the counts belong to
  auto flush = [&] {
    for (int j = 0; j < M.n; ++j) if (cnt[j]) { atomicAdd(&sites[(int64_t)mine * M.n + j], (unsigned long long)cnt[j]); cnt[j] = 0; }
  };
  for (int k = 0; k < PER; ++k) {
    const int64_t s = s0 + k;
    while (c + 1 < hi && r_base[c + 1] <= (uint64_t)s) ++c;
    const int64_t avail = (int64_t)(r_base[c] + (uint64_t)r_len[c]) - s;   // positions of contig c from s on
    const int32_t rk = rank[c - lo];
    if (rk < 0 || (uint64_t)s < r_base[c] || avail <= 0) continue;
    if (rk != mine) { if (mine >= 0) { flush(); sh_mixed = 1; } mine = rk; }
    uint64_t a = k ? w0 >> (4 * k) | w1 << (64 - 4 * k) : w0, b = k ? w1 >> (4 * k) | w2 << (64 - 4 * k) : w1;
    if (avail < 16) { b = 0; a &= ((uint64_t)1 << (4 * avail)) - 1; }
    else if (avail < 32) b &= ((uint64_t)1 << (4 * (avail - 16))) - 1;
    for (int j = 0; j < M.n; ++j)
      cnt[j] += (uint32_t)mmt::fits(a, b, M.m[j].f, M.m[j].len) + (uint32_t)(!combine && mmt::fits(a, b, M.m[j].r, M.m[j].len));
  }
  if (mine >= 0) atomicMax(&sh_rank, mine);
  __syncthreads();
  if (mine >= 0 && mine != sh_rank) sh_mixed = 1;
  __syncthreads();
  if (sh_mixed) { if (mine >= 0) flush(); return; }               // a tile of several listed contigs: every thread adds its own
  for (int j = 0; j < M.n; ++j) {                                  // one contig: the wavefront's sum, the workgroup's, one atomic per motif
    uint32_t v = cnt[j];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((t & 63) == 0 && v) atomicAdd(&acc[j], (unsigned long long)v);
  }
  __syncthreads();
  if (t < M.n && acc[t]) atomicAdd(&sites[(int64_t)sh_rank * M.n + t], acc[t]);
}

struct ContigBytes {                                               // a contig's bytes by its own coordinate (the runs narrowed to what a site can reach)
  EditSeq R; int64_t g0;
  __device__ uint8_t byte(int64_t i) const { return R.byte(g0 + i); }
};
struct SumAdd {                                                    // the sums of a listed contig: [motif][code][covered, modified, N_valid_cov, N_mod]
  unsigned long long* p; int32_t n_codes;
  __device__ void operator()(int32_t motif, int32_t code, bool modified, uint64_t valid, uint64_t mod) const {
    if (!p) return;
    unsigned long long* q = p + ((int64_t)motif * n_codes + code) * 4;
    atomicAdd(q, 1ull); if (modified) atomicAdd(q + 1, 1ull);
    atomicAdd(q + 2, (unsigned long long)valid); if (mod) atomicAdd(q + 3, (unsigned long long)mod);
  }
};
// rows == nullptr: n_rows[i] = the rows of the segment that entry i starts (0 for an entry inside a segment), n_rows[n] = 0 for the scan's total, and the
// sums added; else the rows to rows[pos[i] ...]
__global__ void __launch_bounds__(256) motif_rows_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts, int64_t n, EditSeq R, const uint64_t* __restrict__ r_base,
                                                         const int32_t* __restrict__ r_len, mmd::CodeBases cb, mmt::Motifs M, int64_t min_coverage, double min_frac, int32_t combine,
                                                         int32_t lo, const int32_t* __restrict__ rank, unsigned long long* __restrict__ sums, int32_t* __restrict__ n_rows,
                                                         const int64_t* __restrict__ pos, mmt::Row* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  int k = 0;
  if (i < n && (i == 0 || mmd::key_site(keys[i]) != mmd::key_site(keys[i - 1]))) {
    const int64_t c = mmd::key_contig(keys[i]), q = mmd::key_pos(keys[i]), g0 = (int64_t)r_base[c], len = r_len[c];
    const int64_t a = g0 + std::max<int64_t>(q - mmt::HALO, 0), b = g0 + std::min<int64_t>(q + mmt::HALO + 1, len);
    const ContigBytes ref{R.narrowed((uint64_t)a, (uint64_t)b), g0};
    const SumAdd add{rows ? nullptr : sums + (int64_t)rank[c - lo] * M.n * cb.n * 4, cb.n};
    k = mmt::site_rows(keys, counts, i, n, ref, len, cb, M, min_coverage, min_frac, combine != 0, rows ? rows + pos[i] : nullptr, add);
  }
  if (!rows) n_rows[i] = k;
}
__global__ void __launch_bounds__(256) motif_order_keys_kernel(const mmt::Row* __restrict__ rows, const uint32_t* __restrict__ perm, int64_t n, uint32_t* __restrict__ minor,
                                                               uint64_t* __restrict__ major) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (minor) minor[i] = (uint32_t)rows[i].motif << 2 | (uint32_t)rows[i].code;
  else major[i] = rows[perm[i]].site >> mmd::POS_SHIFT;            // (contig and position from bit 0, sorted over bits [0, 64 - POS_SHIFT): the form that many_units of tests/motif_cases.py holds)
}
}  // namespace

void mod_motifs_run(mm_ctx* ctx, const mm_seqset* ref, const MotifIn& in, MotifResult* out) {
  const std::string w = "mm_mod_motifs: ";
  const mmd::CodeBases cb = mod_table_checks(w, ctx, ref, in.n, in.keys, in.n_codes, in.code_base, in.min_coverage);   // the reference, the codes and the table: mm_mod_finish's
  const int32_t lo = in.contig_lo, hi = in.contig_hi;
  MM_REQUIRE(0 <= lo && lo <= hi && hi <= ref->count(), MM_ERR_ARG, w + "[contig_lo, contig_hi) is no range of the reference's contigs");
  MM_REQUIRE(in.min_frac >= 0.0 && in.min_frac <= 1.0, MM_ERR_ARG, w + "min_frac is not in [0, 1]");
  MM_REQUIRE(in.n_motifs >= 1 && in.n_motifs <= mmt::MAX_MOTIFS && in.motif_off && in.motif_mask && in.motif_pos, MM_ERR_ARG, w + "n_motifs is not in [1, 8]");
  mmt::Motifs M{};
  M.n = in.n_motifs;
  for (int32_t j = 0; j < in.n_motifs; ++j) {
    const std::string item = w + "motif " + std::to_string(j) + ": ";
    const int64_t len = (int64_t)in.motif_off[j + 1] - in.motif_off[j];
    MM_REQUIRE(in.motif_off[j] >= 0 && len >= 1 && len <= mmt::MAX_LEN, MM_ERR_ARG, item + "the length is not in [1, 32]");
    const uint8_t* mask = in.motif_mask + in.motif_off[j];
    for (int64_t i = 0; i < len; ++i) MM_REQUIRE(mask[i] >= 1 && mask[i] <= 15, MM_ERR_ARG, item + "letter " + std::to_string(i) + " is no set of A C G T (a mask of 1 to 15)");
    MM_REQUIRE(in.motif_pos[j] >= 0 && in.motif_pos[j] < len && mmt::mask_base(mask[in.motif_pos[j]]), MM_ERR_ARG, item + "the modified base is not one letter of A C G T inside the motif");
    MM_REQUIRE(mmt::make_motif(mask, (int32_t)len, in.motif_pos[j], &M.m[j]), MM_ERR_ARG, item + "no motif");
    MM_REQUIRE(!in.combine || mmt::own_reverse_complement(M.m[j]), MM_ERR_ARG, item + "combine_strands needs a motif that is its own reverse complement");
  }
  *out = MotifResult{};
  // the group's slice of the table; every entry lies below contig count(), and a key of contig count() = 2^28 would wrap to 0
  auto first_of = [&](int32_t c) { return c < ref->count() ? mmt::lower_entry(in.keys, in.n, mmd::make_key(c, 0, 1, 0)) : in.n; };
  const int64_t k0 = first_of(lo), k1 = first_of(hi), n = k1 - k0;
  if (n <= 0) return;
  std::vector<int32_t> rank((size_t)(hi - lo), -1), listed;
  for (int64_t i = k0; i < k1; ++i) {
    const int32_t c = (int32_t)mmd::key_contig(in.keys[i]);
    if (listed.empty() || listed.back() != c) { rank[(size_t)(c - lo)] = (int32_t)listed.size(); listed.push_back(c); }
  }
  const size_t nl = listed.size(), nm = (size_t)M.n, ncd = (size_t)cb.n;
  hipStream_t st = ctx->stream;
  StageClock<3> clk(getenv("MM_MODS_TIMING") != nullptr, st);
  DBuf<int32_t> d_rank(rank.size());
  DBuf<unsigned long long> d_sites(nl * nm), d_sums(nl * nm * ncd * 4);
  d_rank.upload(rank.data(), rank.size(), st); d_sites.zero(st); d_sums.zero(st);

  clk.start();                                                     // ---- scan: the tiles from the first listed contig's start to the last one's end
  const int64_t tile_a = (int64_t)ref->base[(size_t)listed.front()] / TILE;
  const int64_t tile_b = ceil_div((int64_t)ref->base[(size_t)listed.back()] + ref->len[(size_t)listed.back()], (int64_t)TILE);
  for (int64_t a = tile_a; a < tile_b; a += (int64_t)1 << 24) {
    const unsigned grid = (unsigned)std::min<int64_t>(tile_b - a, (int64_t)1 << 24);
    motif_scan_kernel<<<dim3(grid), dim3(T), 0, st>>>(ref->packed.p, (int64_t)ref->packed.n, edit_seq(ref), ref->d_base.p, ref->d_len.p, lo, hi, d_rank.p, M, in.combine, a, d_sites.p);
    MM_KERNEL_CHECK();
  }
  clk.stop(0);

  clk.start();                                                     // ---- sites: count, scan, emit
  const size_t k = (size_t)n;
  DBuf<uint64_t> d_keys(k); DBuf<uint32_t> d_counts(k); DBuf<int32_t> d_nrows(k + 1); DBuf<int64_t> d_pos(k + 1); DBuf<uint8_t> tmp;
  d_keys.upload(in.keys + k0, k, st); d_counts.upload(in.counts + k0, k, st);
  auto rows_pass = [&](mmt::Row* rows) {
    motif_rows_kernel<<<dim3(flat_grid(n + 1)), dim3(256), 0, st>>>(d_keys.p, d_counts.p, n, edit_seq(ref), ref->d_base.p, ref->d_len.p, cb, M, in.min_coverage, in.min_frac, in.combine, lo,
                                                                   d_rank.p, d_sums.p, d_nrows.p, d_pos.p, rows);
    MM_KERNEL_CHECK();
  };
  rows_pass(nullptr);
  exclusive_scan(tmp, d_nrows.p, d_pos.p, k + 1, st);
  int64_t total = 0;
  d_pos.download(&total, 1, st, k);
  MM_HIP(mm::stream_sync(st));
  MM_REQUIRE(total < ((int64_t)1 << 32), MM_ERR_LIMIT, w + "2^32 rows or more in one group");
  std::vector<mmt::Row> rows;
  std::vector<uint32_t> perm;
  if (total > 0) {
    DBuf<mmt::Row> d_rows((size_t)total);
    rows_pass(d_rows.p);
    clk.stop(1);
    clk.start();
    if (in.combine) {                                              // the units' order: stable by (motif, code), then stable by the site
      const size_t r = (size_t)total;
      DBuf<uint32_t> minor(r), minor_out(r), iota(r), p1(r), p2(r); DBuf<uint64_t> major(r), major_out(r);
      motif_order_keys_kernel<<<dim3(flat_grid(total)), dim3(256), 0, st>>>(d_rows.p, nullptr, total, minor.p, nullptr); MM_KERNEL_CHECK();
      fill_iota(iota.p, total, st);
      sort_pairs(tmp, minor.p, minor_out.p, iota.p, p1.p, r, 0, 5, st);
      motif_order_keys_kernel<<<dim3(flat_grid(total)), dim3(256), 0, st>>>(d_rows.p, p1.p, total, nullptr, major.p); MM_KERNEL_CHECK();
      sort_pairs(tmp, major.p, major_out.p, p1.p, p2.p, r, 0, 64 - mmd::POS_SHIFT, st);
      perm = p2.to_host(st);
    }
    rows = d_rows.to_host(st);
  } else { clk.stop(1); clk.start(); }
  const std::vector<unsigned long long> sites = d_sites.to_host(st), sums = d_sums.to_host(st);
  MM_HIP(mm::stream_sync(st));
  clk.stop(2);
  for (size_t i = 0; i < rows.size(); ++i) {
    const mmt::Row& r = rows[perm.empty() ? i : (size_t)perm[i]];
    out->site.push_back(r.site); out->motif.push_back(r.motif); out->code.push_back(r.code);
    out->n_mod.push_back(r.n_mod); out->n_canonical.push_back(r.n_canonical); out->n_other.push_back(r.n_other); out->n_fail.push_back(r.n_fail);
  }
  for (size_t l = 0; l < nl; ++l)
    for (size_t j = 0; j < nm; ++j)
      for (size_t c = 0; c < ncd; ++c) {
        if (cb.b[c] != M.m[j].base) continue;
        const unsigned long long* s = &sums[((l * nm + j) * ncd + c) * 4];
        out->s_contig.push_back(listed[l]); out->s_motif.push_back((int32_t)j); out->s_code.push_back((int32_t)c);
        out->sums.push_back((int64_t)sites[l * nm + j]);
        for (int x = 0; x < 4; ++x) out->sums.push_back((int64_t)s[x]);
      }
  if (clk.on)
    fprintf(stderr, "MM_MODS_TIMING motifs: scan %.3f ms, sites %.3f ms, order and copies %.3f ms; contigs [%d, %d), %lld tiles, %lld entries, %zu listed contigs, %d motifs, %zu rows\n",
            clk.ms[0], clk.ms[1], clk.ms[2], lo, hi, (long long)(tile_b - tile_a), (long long)n, nl, M.n, out->site.size());
}

}  // namespace mm
