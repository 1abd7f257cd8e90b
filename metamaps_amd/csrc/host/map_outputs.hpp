// The side outputs of a batch of mapDirectly (the rows of side_files.hpp: PREFIX.editDistances, .paf, .bam and the four read files of reads_out.hpp) and the device calls they need, and the run's
// pileup (PREFIX.pileup, .pileup.contigs), alleles (PREFIX.vcf), consensus (PREFIX.consensus.fa, .consensus.tsv), modification counts (PREFIX.bedmethyl, .motifs.*) and
// depth profile (PREFIX.depth.bedgraph, .depth.windows, .depth.contigs) and error profile (PREFIX.errorProfile.*), which every batch adds to.  The text and
// byte rules are in edit_dist.hpp, paf_out.hpp, bam_out.hpp, pileup_out.hpp, vcf_out.hpp, consensus_out.hpp, mods_out.hpp, motif_out.hpp, depth_out.hpp and errprof_out.hpp,
// which call nothing; everything of a batch runs on the context that mapped it, the last merge and the finish of the pileup, of the alleles, of the consensus
// and of the modification counts, the depth profile and the error profile's rows on the first device.
#pragma once
#include "bam_out.hpp"
#include "bam_sort_out.hpp"
#include "classify_run.hpp"
#include "cli_device.hpp"
#include "consensus_out.hpp"
#include "depth_out.hpp"
#include "edit_dist.hpp"
#include "errprof_out.hpp"
#include "mods_out.hpp"
#include "motif_out.hpp"
#include "paf_out.hpp"
#include "pileup_out.hpp"
#include "reads_out.hpp"
#include "side_files.hpp"
#include "vcf_out.hpp"
#include <memory>

namespace {

// a batch's reads on the device, held by one owner: destroyed once, when the last output that needs them is made (or when that owner goes)
struct SeqsetDestroy { void operator()(mm_seqset* s) const { mm_seqset_destroy(s); } };
using ReadsPtr = std::unique_ptr<mm_seqset, SeqsetDestroy>;

using SideBytes = std::array<std::string, N_SIDE>;               // what one batch adds to every side file

// `raw` as BGZF members (mm_bgzf_deflate: blocks of 65 280 bytes, each a member of its own, so what is deflated piece by piece concatenates)
void bgzf_members(mm_ctx* ctx, const std::string& raw, std::string& gz, const char* what) {
  gz.resize((size_t)mm_bgzf_deflate_bound((int64_t)raw.size()));
  int64_t nbytes = 0; int32_t nblocks = 0;
  ck(ctx, mm_bgzf_deflate(ctx, (const uint8_t*)raw.data(), (int64_t)raw.size(), (uint8_t*)&gz[0], (int64_t)gz.size(), &nbytes, &nblocks), what);
  gz.resize((size_t)nbytes);
}
// the header of PREFIX.bam (bam_out.hpp) as BGZF members
std::string bam_header_members(mm_ctx* ctx, const std::vector<std::string>& cname, const std::vector<int>& clen) {
  std::string gz;
  bgzf_members(ctx, bam_header(cname, clen), gz, "deflate the BAM header");
  return gz;
}

// The device's calls of --pileup and of --vcf in one shape, for the three functions below: a pileup table has one-word keys, a VCF table two.
// fetch: the rows behind a handle, which goes.
struct PileupCalls {
  using Table = mm_pileup;
  static constexpr const char* events_what = "pileup events"; static constexpr const char* merge_what = "pileup merge";
  static constexpr auto events = mm_pileup_events_q;
  static int merge(mm_ctx* ctx, const VariantRows& v, Table** t) { return mm_pileup_merge(ctx, (int64_t)v.w0.size(), v.w0.data(), v.counts.data(), t); }
  static void fetch(Table* t, VariantRows& v) {
    int64_t n = 0;
    mm_pileup_sizes(t, &n); v.resize((size_t)n, false); mm_pileup_fetch(t, v.w0.data(), v.counts.data()); mm_pileup_destroy(t);
  }
};
struct VcfCalls {
  using Table = mm_vcf;
  static constexpr const char* events_what = "vcf events"; static constexpr const char* merge_what = "vcf merge";
  static constexpr auto events = mm_vcf_events_q;
  static int merge(mm_ctx* ctx, const VariantRows& v, Table** t) { return mm_vcf_merge(ctx, (int64_t)v.w0.size(), v.w0.data(), v.w1.data(), v.counts.data(), t); }
  static void fetch(Table* t, VariantRows& v) {
    int64_t n = 0;
    mm_vcf_sizes(t, &n); v.resize((size_t)n, true); mm_vcf_fetch(t, v.w0.data(), v.w1.data(), v.counts.data()); mm_vcf_destroy(t);
  }
};
// --mods in the same shape: one-word keys; the int32 behind `use` is the ML threshold where the other two take the base-quality floor
struct ModCalls {
  using Table = mm_mod;
  static constexpr const char* events_what = "modification events"; static constexpr const char* merge_what = "modification merge";
  static constexpr auto events = mm_mod_events;
  static int merge(mm_ctx* ctx, const VariantRows& v, Table** t) { return mm_mod_merge(ctx, (int64_t)v.w0.size(), v.w0.data(), v.counts.data(), t); }
  static void fetch(Table* t, VariantRows& v) {
    int64_t n = 0;
    mm_mod_sizes(t, &n); v.resize((size_t)n, false); mm_mod_fetch(t, v.w0.data(), v.counts.data()); mm_mod_destroy(t);
  }
};
// rows and their sums through the output's merge, which leaves them unique and ascending
template <class C> void merge_rows(mm_ctx* ctx, VariantRows& v) {
  typename C::Table* t = nullptr;
  ck(ctx, C::merge(ctx, v, &t), C::merge_what);
  C::fetch(t, v);
}
// --pileup and --vcf, per batch: the events (alleles) of the primary aligned records (use) counted on the context that mapped the batch, appended to the
// file's accumulator; above merge_pairs rows the accumulator is replaced by its merge.  min_base_quality: --min-base-quality's floor (0: none)
template <class C> void add_batch(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const BamFields& F, const BatchAlignment& al, const std::vector<uint8_t>& use,
                                  int32_t min_base_quality, size_t merge_pairs, VariantAcc& acc) {
  typename C::Table* t = nullptr;
  ck(ctx, C::events(ctx, reads, reference, (int64_t)use.size(), F.read.data(), F.strand.data(), F.contig.data(), al.dist.data(), al.first.data(), al.op_off.data(), al.ops.data(),
                    use.data(), min_base_quality, &t), C::events_what);
  VariantRows got;
  C::fetch(t, got);
  std::lock_guard<std::mutex> lk(acc.m);
  VariantRows& a = acc.rows;
  a.w0.insert(a.w0.end(), got.w0.begin(), got.w0.end()); a.w1.insert(a.w1.end(), got.w1.begin(), got.w1.end()); a.counts.insert(a.counts.end(), got.counts.begin(), got.counts.end());
  if (a.w0.size() > merge_pairs) merge_rows<C>(ctx, a);
}
void write_or_die(const std::string& path, const std::string& text) {
  FILE* out = fopen(path.c_str(), "wb");
  if (!out || fwrite(text.data(), 1, text.size(), out) != text.size() || fclose(out) != 0) die("Error writing " + path);
}
// --pileup, after the last batch of a query file: one merge, one mm_pileup_finish against the reference of `ctx`, and the two files
void pileup_write(mm_ctx* ctx, const mm_seqset* reference, VariantRows& v, const Intervals& iv, const PileupOpts& po, const std::string& prefix, const std::vector<std::string>& cname,
                  const std::vector<int>& clen) {
  merge_rows<PileupCalls>(ctx, v);
  mm_pileup_result* r = nullptr;
  ck(ctx, mm_pileup_finish(ctx, reference, (int64_t)v.w0.size(), v.w0.data(), v.counts.data(), (int64_t)iv.contig.size(), iv.contig.data(), iv.first.data(), iv.last.data(),
                           po.min_count, po.min_frac, &r), "pileup");
  int64_t n_sites = 0, n_contigs = 0;
  mm_pileup_result_sizes(r, &n_sites, &n_contigs);
  std::vector<uint64_t> key((size_t)n_sites); std::vector<uint32_t> count((size_t)n_sites), depth((size_t)n_sites); std::vector<uint8_t> ref_byte((size_t)n_sites);
  std::vector<int64_t> alignments((size_t)n_contigs), covered((size_t)n_contigs), sum_depth((size_t)n_contigs);
  mm_pileup_result_fetch_sites(r, key.data(), count.data(), depth.data(), ref_byte.data());
  mm_pileup_result_fetch_contigs(r, alignments.data(), covered.data(), sum_depth.data());
  mm_pileup_result_destroy(r);
  if (n_contigs != (int64_t)cname.size()) die("internal error: the pileup's contigs and the reference's differ in number");
  write_or_die(prefix + ".pileup", pileup_text(key, count, depth, ref_byte, cname));
  write_or_die(prefix + ".pileup.contigs", pileup_contigs_text(alignments, covered, sum_depth, cname, clen));
}
// --mods, after the last batch of a query file: one merge, one mm_mod_finish against the reference of `ctx`, and the file
void mods_write(mm_ctx* ctx, const mm_seqset* reference, VariantRows& v, const ModsOpts& mo, const std::string& prefix, const std::vector<std::string>& cname) {
  merge_rows<ModCalls>(ctx, v);
  mm_mod_result* r = nullptr;
  ck(ctx, mm_mod_finish(ctx, reference, (int64_t)v.w0.size(), v.w0.data(), v.counts.data(), mo.n_codes, mo.code_base, mo.min_coverage, &r), "modification rows");
  int64_t n = 0;
  mm_mod_result_sizes(r, &n);
  std::vector<uint64_t> site((size_t)n), n_mod((size_t)n), n_canonical((size_t)n), n_other((size_t)n), n_fail((size_t)n);
  mm_mod_result_fetch(r, site.data(), n_mod.data(), n_canonical.data(), n_other.data(), n_fail.data());
  mm_mod_result_destroy(r);
  write_or_die(prefix + ".bedmethyl", bedmethyl_text(mo, site, n_mod, n_canonical, n_other, n_fail, cname));
}
// --mod-motifs, behind mods_write (which has merged the table): the groups of consensus_out.hpp over the contigs with an entry, the entries of a group cut out by
// key, one mm_mod_motifs per group on `ctx`, and the two files
void motifs_write(mm_ctx* ctx, const mm_seqset* reference, const VariantRows& v, const ModsOpts& mo, const MotifOpts& mt, int64_t group_bases, const std::string& prefix,
                  const std::vector<std::string>& cname, const std::vector<int>& clen) {
  std::vector<int32_t> listed;
  for (uint64_t key : v.w0) if (listed.empty() || listed.back() != (int32_t)mmd::key_contig(key)) listed.push_back((int32_t)mmd::key_contig(key));
  FILE* fb = fopen((prefix + ".motifs.bedmethyl").c_str(), "wb");
  FILE* ft = fopen((prefix + ".motifs.tsv").c_str(), "wb");
  if (!fb || !ft) die("Error writing " + prefix + ".motifs.bedmethyl / .motifs.tsv");
  auto put = [&](FILE* f, std::string& t) { if (fwrite(t.data(), 1, t.size(), f) != t.size()) die("Error writing " + prefix + ".motifs.bedmethyl / .motifs.tsv"); t.clear(); };
  std::string bed, tsv = motif_tsv_header();                      // (appended to as the groups come)
  std::vector<int64_t> total;
  std::vector<uint64_t> site, n_mod, n_canonical, n_other, n_fail; std::vector<int32_t> motif, code, s_contig, s_motif, s_code; std::vector<int64_t> sums;
  for (const ConsGroupRange& g : cons_groups(clen, listed, group_bases)) {
    const size_t r0 = (size_t)(std::lower_bound(v.w0.begin(), v.w0.end(), mmd::make_key(g.lo, 0, 1, 0)) - v.w0.begin());
    const size_t r1 = (size_t)g.hi < clen.size() ? (size_t)(std::lower_bound(v.w0.begin(), v.w0.end(), mmd::make_key(g.hi, 0, 1, 0)) - v.w0.begin())
                                                 : v.w0.size();    // (a key of contig 2^28 would wrap to 0)
    mm_motif_result* r = nullptr;
    ck(ctx, mm_mod_motifs(ctx, reference, g.lo, g.hi, (int64_t)(r1 - r0), v.w0.data() + r0, v.counts.data() + r0, mo.n_codes, mo.code_base, mt.n, mt.off.data(), mt.mask.data(),
                          mt.pos.data(), mo.min_coverage, mt.min_frac, mt.combine ? 1 : 0, &r), "modification motifs");
    int64_t n = 0, ns = 0;
    mm_motif_result_sizes(r, &n, &ns);
    for (auto* x : {&site, &n_mod, &n_canonical, &n_other, &n_fail}) x->resize((size_t)n);
    motif.resize((size_t)n); code.resize((size_t)n); s_contig.resize((size_t)ns); s_motif.resize((size_t)ns); s_code.resize((size_t)ns); sums.resize((size_t)ns * MM_MOTIF_SUMS);
    mm_motif_result_fetch_rows(r, site.data(), motif.data(), code.data(), n_mod.data(), n_canonical.data(), n_other.data(), n_fail.data());
    mm_motif_result_fetch_summary(r, s_contig.data(), s_motif.data(), s_code.data(), sums.data());
    mm_motif_result_destroy(r);
    motif_bedmethyl_text(mo, mt, site, motif, code, n_mod, n_canonical, n_other, n_fail, cname, bed);
    motif_tsv_text(mo, mt, s_contig, s_motif, s_code, sums, cname, total, tsv);
    put(fb, bed); put(ft, tsv);
  }
  motif_tsv_totals(mo, mt, total, tsv);
  put(ft, tsv);
  if (fclose(fb) != 0 || fclose(ft) != 0) die("Error writing " + prefix + ".motifs.bedmethyl / .motifs.tsv");
}
// --vcf, after the last batch of a query file and the merge of its rows: one mm_vcf_finish against the reference of `ctx` over the file's intervals, and the file
void vcf_write(mm_ctx* ctx, const mm_seqset* reference, const VariantRows& v, const Intervals& iv, const VcfOpts& vo, int min_base_quality, const std::string& prefix,
               const std::vector<std::string>& cname, const std::vector<int>& clen) {
  mm_vcf_result* r = nullptr;
  ck(ctx, mm_vcf_finish(ctx, reference, (int64_t)v.w0.size(), v.w0.data(), v.w1.data(), v.counts.data(), (int64_t)iv.contig.size(), iv.contig.data(), iv.first.data(), iv.last.data(),
                        vo.min_count, vo.min_frac, &r), "vcf");
  int64_t n = 0;
  mm_vcf_result_sizes(r, &n);
  std::vector<uint64_t> w0((size_t)n), w1((size_t)n); std::vector<uint32_t> count((size_t)n), depth((size_t)n); std::vector<uint8_t> window((size_t)n * MM_VCF_WINDOW);
  mm_vcf_result_fetch(r, w0.data(), w1.data(), count.data(), depth.data(), window.data());
  mm_vcf_result_destroy(r);
  write_or_die(prefix + ".vcf", vcf_header(cname, clen, min_base_quality) + vcf_lines(w0, w1, count, depth, window, cname));
}
// --consensus, after the last batch of a query file and the merge of its rows: the intervals in contig order, the groups of consensus_out.hpp, the rows of
// a group cut out by key, one mm_consensus per group on `ctx`, and the two files appended to as the groups come
void consensus_write(mm_ctx* ctx, const mm_seqset* reference, const VariantRows& v, const Intervals& iv, const ConsOpts& co, int64_t group_bases, const std::string& prefix,
                     const std::vector<std::string>& cname, const std::vector<int>& clen) {
  const std::vector<size_t> order = cons_interval_order(iv.contig);
  std::vector<int32_t> ic(order.size()); std::vector<int64_t> i0(order.size()), i1(order.size());
  for (size_t k = 0; k < order.size(); ++k) { ic[k] = iv.contig[order[k]]; i0[k] = iv.first[order[k]]; i1[k] = iv.last[order[k]]; }
  FILE* fa = fopen((prefix + ".consensus.fa").c_str(), "wb");
  FILE* tsv = fopen((prefix + ".consensus.tsv").c_str(), "wb");
  if (!fa || !tsv) die("Error writing " + prefix + ".consensus.fa / .consensus.tsv");
  auto put = [&](FILE* f, const char* p, size_t n) { if (fwrite(p, 1, n, f) != n) die("Error writing " + prefix + ".consensus.fa / .consensus.tsv"); };
  const std::string head = cons_tsv_header();
  put(tsv, head.data(), head.size());
  std::vector<int32_t> contig, written; std::vector<int64_t> stats, text_off; std::vector<uint8_t> text;
  for (const ConsGroupRange& g : cons_groups(clen, ic, group_bases)) {
    const size_t r0 = (size_t)(std::lower_bound(v.w0.begin(), v.w0.end(), mmp::make_key(g.lo, 0, 0)) - v.w0.begin());
    const size_t r1 = (size_t)(std::lower_bound(v.w0.begin(), v.w0.end(), mmp::make_key(g.hi, 0, 0)) - v.w0.begin());
    const size_t v0 = (size_t)(std::lower_bound(ic.begin(), ic.end(), g.lo) - ic.begin()), v1 = (size_t)(std::lower_bound(ic.begin(), ic.end(), g.hi) - ic.begin());
    struct mm_consensus* r = nullptr;
    ck(ctx, mm_consensus(ctx, reference, g.lo, g.hi, (int64_t)(r1 - r0), v.w0.data() + r0, v.w1.data() + r0, v.counts.data() + r0, (int64_t)(v1 - v0), ic.data() + v0, i0.data() + v0,
                         i1.data() + v0, co.min_depth, co.min_frac, co.min_called, CONS_LINE_WIDTH, &r), "consensus");
    int64_t n = 0, nw = 0, bytes = 0;
    mm_consensus_sizes(r, &n, &nw, &bytes);
    contig.resize((size_t)n); stats.resize((size_t)n * MM_CONS_STATS); written.resize((size_t)nw); text_off.resize((size_t)nw + 1); text.resize((size_t)bytes);
    mm_consensus_fetch_contigs(r, contig.data(), stats.data());
    mm_consensus_fetch_text(r, written.data(), text_off.data(), text.data());
    mm_consensus_destroy(r);
    std::string rows;
    for (size_t k = 0; k < (size_t)n; ++k) cons_tsv_row(cname[(size_t)contig[k]], clen[(size_t)contig[k]], &stats[k * MM_CONS_STATS], rows);
    put(tsv, rows.data(), rows.size());
    for (size_t k = 0; k < (size_t)nw; ++k) {
      const std::string name = cons_fasta_name(cname[(size_t)written[k]]);
      put(fa, name.data(), name.size());
      put(fa, (const char*)text.data() + text_off[k], (size_t)(text_off[k + 1] - text_off[k]));
    }
  }
  if (fclose(fa) != 0 || fclose(tsv) != 0) die("Error writing " + prefix + ".consensus.fa / .consensus.tsv");
}
// --depth, after the last batch of a query file: one mm_depth_profile on `ctx` over the file's intervals and the contigs' lengths, and the three files
void depth_write(mm_ctx* ctx, const Intervals& iv, const DepthOpts& dp, const std::string& prefix, const std::vector<std::string>& cname, const std::vector<int>& clen) {
  const std::vector<int64_t> len(clen.begin(), clen.end());
  mm_depth* r = nullptr;
  ck(ctx, mm_depth_profile(ctx, (int64_t)len.size(), len.data(), (int64_t)iv.contig.size(), iv.contig.data(), iv.first.data(), iv.last.data(), dp.window, dp.n_thresholds,
                           dp.thresholds, &r), "depth profile");
  int64_t n_runs = 0, n_contigs = 0, n_windows = 0;
  mm_depth_sizes(r, &n_runs, &n_contigs, &n_windows);
  std::vector<int32_t> run_contig((size_t)n_runs), contig((size_t)n_contigs); std::vector<int64_t> start((size_t)n_runs), end((size_t)n_runs); std::vector<uint32_t> depth((size_t)n_runs);
  std::vector<int64_t> win_off((size_t)n_contigs + 1), stats((size_t)n_contigs * (size_t)(MM_DEPTH_STATS + dp.n_thresholds)), sum((size_t)n_windows), covered((size_t)n_windows);
  mm_depth_fetch_runs(r, run_contig.data(), start.data(), end.data(), depth.data());
  mm_depth_fetch_contigs(r, contig.data(), win_off.data(), stats.data());
  mm_depth_fetch_windows(r, sum.data(), covered.data());
  mm_depth_destroy(r);
  write_or_die(prefix + ".depth.bedgraph", depth_bedgraph_text(run_contig, start, end, depth, cname));
  write_or_die(prefix + ".depth.windows", depth_windows_text(contig, win_off, sum, covered, dp.window, cname, clen));
  write_or_die(prefix + ".depth.contigs", depth_contigs_text(dp, contig, stats, cname, clen));
}
// --error-profile, per batch: the counters, columns and identity keys of the primary aligned records (use) walked on the context that mapped the batch
void errprof_add_batch(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, const BamFields& F, const BatchAlignment& al, const std::vector<uint8_t>& use, ErrprofAcc& acc) {
  uint64_t counters[MM_ERRPROF_COUNTERS];
  std::vector<int32_t> cols(use.size() * MM_ERRPROF_COLS); std::vector<uint64_t> key(use.size());
  ck(ctx, mm_errprof_events(ctx, reads, reference, (int64_t)use.size(), F.read.data(), F.strand.data(), F.contig.data(), al.dist.data(), al.first.data(), al.op_off.data(), al.ops.data(),
                            use.data(), counters, cols.data(), key.data()), "error profile");
  acc.add(counters, key, cols);
}
// --error-profile, after the last batch of a query file: one mm_errprof_finish on `ctx` over the file's keys and columns, and the four files
void errprof_write(mm_ctx* ctx, const ErrprofAcc& acc, const std::string& prefix, const std::vector<std::string>& cname, const std::vector<int>& clen) {
  mm_errprof* r = nullptr;
  ck(ctx, mm_errprof_finish(ctx, (int64_t)cname.size(), (int64_t)acc.key.size(), acc.key.data(), acc.cols.data(), &r), "error profile rows");
  int64_t n = 0;
  mm_errprof_sizes(r, &n);
  std::vector<int32_t> contig((size_t)n); std::vector<int64_t> stats((size_t)(n + 1) * MM_ERRPROF_STATS);
  mm_errprof_fetch(r, contig.data(), stats.data());
  mm_errprof_destroy(r);
  if (!acc.key.empty() && !errprof_any_quality(acc.counters))
    std::cout << "INFO, --error-profile: no read of " << prefix << " carried a base quality: " << prefix << ".errorProfile.qualities has the row `none` alone (--base-qualities keeps them)\n";
  write_or_die(prefix + ".errorProfile.substitutions", errprof_substitutions_text(acc.counters));
  write_or_die(prefix + ".errorProfile.indels", errprof_indels_text(acc.counters));
  write_or_die(prefix + ".errorProfile.qualities", errprof_qualities_text(acc.counters));
  write_or_die(prefix + ".errorProfile.contigs", errprof_contigs_text(contig, stats, cname, clen));
}
// the run's accumulators, one set per query file, and what is written from them after the last batch (every pileup before the first VCF).  The alleles are
// accumulated (vcf_on) for --vcf and for --consensus, merged once, and written as PREFIX.vcf under --vcf alone
struct RunVariants {
  struct File { Intervals iv; VariantAcc pile, vcf, mods; ErrprofAcc errprof; };
  bool pileup_on = false, vcf_on = false, vcf_file = false, cons_on = false, mods_on = false, depth_on = false, errprof_on = false;
  std::deque<File> files;
  SortedBams sorted;                                             // --bam-sorted: the runs of every query file (bam_sort_out.hpp)
  void resize(bool pileup, bool vcf, bool cons, bool mods, bool depth, bool bam_sorted, bool errprof, size_t n_files) {
    pileup_on = pileup; vcf_on = vcf || cons; vcf_file = vcf; cons_on = cons; mods_on = mods; depth_on = depth; errprof_on = errprof;
    sorted.on = bam_sorted;
    if (bam_sorted) sorted.files.resize(n_files);
    if (pileup_on || vcf_on || mods_on || depth_on || errprof_on) files.resize(n_files);
  }
  VariantAcc* pile(size_t f) { return pileup_on ? &files[f].pile : nullptr; }
  VariantAcc* vcf(size_t f) { return vcf_on ? &files[f].vcf : nullptr; }
  VariantAcc* mods(size_t f) { return mods_on ? &files[f].mods : nullptr; }
  ErrprofAcc* errprof(size_t f) { return errprof_on ? &files[f].errprof : nullptr; }
  Intervals* intervals(size_t f) { return files.empty() ? nullptr : &files[f].iv; }
  void write(mm_ctx* ctx, const mm_seqset* reference, const PileupOpts& po, const VcfOpts& vo, const ConsOpts& co, const ModsOpts& mo, const MotifOpts& mt, const DepthOpts& dp,
             int min_base_quality, int64_t cons_group_bases, int64_t motif_group_bases, int64_t bam_sort_window, const std::vector<std::string>& prefixes,
             const std::vector<std::string>& cname, const std::vector<int>& clen) {
    for (size_t fi = 0; pileup_on && fi < files.size(); ++fi) pileup_write(ctx, reference, files[fi].pile.rows, files[fi].iv, po, prefixes[fi], cname, clen);
    for (size_t fi = 0; depth_on && fi < files.size(); ++fi) depth_write(ctx, files[fi].iv, dp, prefixes[fi], cname, clen);
    for (size_t fi = 0; errprof_on && fi < files.size(); ++fi) errprof_write(ctx, files[fi].errprof, prefixes[fi], cname, clen);
    for (size_t fi = 0; mods_on && fi < files.size(); ++fi) {
      mods_write(ctx, reference, files[fi].mods.rows, mo, prefixes[fi], cname);
      if (mt.on) motifs_write(ctx, reference, files[fi].mods.rows, mo, mt, motif_group_bases, prefixes[fi], cname, clen);
    }
    for (size_t fi = 0; vcf_on && fi < files.size(); ++fi) {
      merge_rows<VcfCalls>(ctx, files[fi].vcf.rows);
      if (vcf_file) vcf_write(ctx, reference, files[fi].vcf.rows, files[fi].iv, vo, min_base_quality, prefixes[fi], cname, clen);
      if (cons_on) consensus_write(ctx, reference, files[fi].vcf.rows, files[fi].iv, co, cons_group_bases, prefixes[fi], cname, clen);
    }
    if (sorted.on) {
      std::string head;
      bgzf_members(ctx, bam_header(cname, clen, true), head, "deflate the sorted BAM header");
      for (size_t fi = 0; fi < sorted.files.size(); ++fi) sorted_bam_write(ctx, sorted.files[fi], prefixes[fi], head, clen, bam_sort_window);
    }
  }
};

// --extract-*, --deplete-taxa: what a batch's read files need beside the batch itself
struct ReadsOut { ReadsOutOpts opts; ContigHits hits; };
// ... per batch: the reads each file takes (reads_out.hpp) written as FASTQ / FASTA records and deflated on the context that holds the batch's reads
// (mm_reads_encode); only the members come back.  A batch without a selected read adds nothing to the file.
void extract_batch(mm_ctx* ctx, const mm_seqset* reads, const ReadsOut& ro, const std::vector<mm_map_record>& rec, const std::vector<std::string>& names,
                   const std::vector<int64_t>& off, const std::string& text, SideBytes& out) {
  std::vector<int32_t> contig(rec.size());
  for (size_t i = 0; i < rec.size(); ++i) contig[i] = rec[i].ref_contig;
  const std::vector<int32_t> primary = primary_contigs(off, contig, bam_line_q(text, rec.size()));
  for (int f = 0; f < N_EXTRACT; ++f) {
    if (!ro.opts.on[(size_t)f]) continue;
    std::string& members = out[(size_t)kExtract[f].side];
    members.clear();
    const std::vector<int32_t> sel = extract_selection(f, primary, ro.hits);
    if (sel.empty()) continue;
    std::vector<int64_t> name_off(sel.size() + 1, 0); std::string all;
    for (size_t i = 0; i < sel.size(); ++i) { all += names[(size_t)sel[i]]; name_off[i + 1] = (int64_t)all.size(); }
    mm_reads_text* t = nullptr;
    ck(ctx, mm_reads_encode(ctx, reads, (int64_t)sel.size(), sel.data(), name_off.data(), all.data(), ro.opts.with_qual ? 1 : 0, 0, &t), (std::string("--") + kExtract[f].flag).c_str());
    int64_t n_records = 0, raw = 0, bytes = 0;
    mm_reads_text_sizes(t, &n_records, &raw, &bytes);
    members.resize((size_t)bytes);
    if (bytes) mm_reads_text_fetch(t, (uint8_t*)&members[0]);
    mm_reads_text_destroy(t);
  }
}

// The side outputs of one batch, in the two steps the order of a batch's device calls leaves: the alignment needs the mapping, which goes before the
// lines are formatted; the BAM records need the formatted lines (their mapping qualities are read from the text).  One alignment serves all three files.
struct BatchSideOutputs {
  const SideSet& on;
  BatchAlignment al;
  VariantAcc* pile = nullptr;                                    // --pileup: the accumulator of the batch's query file
  size_t pile_merge_pairs = 0;
  VariantAcc* vcf = nullptr;                                     // --vcf, --consensus: the accumulator of the batch's query file
  size_t vcf_merge_pairs = 0;
  Intervals* iv = nullptr;                                       // --pileup, --vcf, --consensus, --depth: the contributing alignments of the batch's query file
  int32_t min_base_quality = 0;                                  // --min-base-quality: the floor of the pileup's events and of the alleles
  VariantAcc* mods = nullptr;                                    // --mods: the accumulator of the batch's query file (the base-quality floor does not touch its counts)
  size_t mods_merge_pairs = 0;
  int32_t min_ml = 0;                                            // --mod-min-ml: the ML byte below which a call counts as failed
  bool depth = false;                                            // --depth: the intervals alone (no accumulator, no traceback: first and last come with the distances)
  SortedRun* sorted = nullptr;                                   // --bam-sorted: the batch's sorted run (bam_sort_out.hpp)
  ErrprofAcc* errprof = nullptr;                                 // --error-profile: the accumulator of the batch's query file (a third user of the reads' qualities)
  const ReadsOut* extract = nullptr;                             // --extract-*, --deplete-taxa: the read files (they keep the reads until from_text, and need no alignment)

  // while the mapping lives: d, first, last (and the runs, where .paf or .bam want them) fetched once -> the lines of .editDistances and .paf.
  // The reads go here unless .bam needs them for SEQ, the pileup or the VCF for their mismatched and inserted bases, or --mods for their calls; --depth reads
  // none of them but keeps them until from_text, which does nothing without them.
  // Nothing happens without reads (no side file was asked for), and nothing here for the read files alone: they need no alignment, and their reads wait.
  void from_mapping(mm_ctx* ctx, const mm_mapping* m, ReadsPtr& reads, const mm_seqset* reference, float pi, const std::vector<mm_map_record>& rec,
                    const std::vector<std::string>& names, const std::vector<int>& lens, const std::vector<int64_t>& off, const std::vector<std::string>& cname,
                    const std::vector<int>& clen, SideBytes& out) {
    if (!reads || !on[SIDE_EDIT]) return;
    const size_t n = rec.size();
    if (on[SIDE_PAF] || on[SIDE_BAM] || sorted || pile || vcf || mods || errprof) {
      mm_alignment* a = nullptr;
      ck(ctx, mm_mapping_align(ctx, m, reads.get(), reference, pi, &a), "alignments");
      int64_t n_jobs = 0, n_ops = 0;
      mm_alignment_sizes(a, &n_jobs, &n_ops);
      if (n_jobs != (int64_t)n) die("internal error: alignments and records differ in number");
      al.dist.resize(n); al.first.resize(n); al.last.resize(n); al.op_off.resize(n + 1); al.ops.resize((size_t)n_ops);
      mm_alignment_fetch(a, al.dist.data(), al.first.data(), al.last.data(), al.op_off.data(), al.ops.data());
      mm_alignment_destroy(a);
    } else {                                                       // --edit-distance alone: the distances without the traceback
      al.dist.resize(n); al.first.resize(n); al.last.resize(n);
      ck(ctx, mm_mapping_edit_distances(ctx, m, reads.get(), reference, pi, al.dist.data(), al.first.data(), al.last.data(), (int64_t)n), "edit distances");
    }
    edit_distance_text(al.dist.data(), al.first.data(), al.last.data(), names, off, rec, cname, out[SIDE_EDIT]);
    if (on[SIDE_PAF]) paf_text(al, names, lens, off, rec, cname, clen, out[SIDE_PAF]);
    if (!on[SIDE_BAM] && !sorted && !pile && !vcf && !mods && !depth && !errprof && !extract) reads.reset();
  }

  // once the lines are formatted: the batch's BAM records as BGZF members, encoded and deflated on the device, and its pileup events and alleles (all go by
  // bam_fields' primary record, which needs the lines); the reads, kept for this, go
  void from_text(mm_ctx* ctx, ReadsPtr& reads, const mm_seqset* reference, const std::vector<mm_map_record>& rec, const std::vector<std::string>& names,
                 const std::vector<int64_t>& off, const std::string& text, SideBytes& out) {
    if (!reads) return;
    if (extract) extract_batch(ctx, reads.get(), *extract, rec, names, off, text, out);   // (every read of the batch: one without a line is `unmapped`)
    std::string& members = out[SIDE_BAM];
    members.clear();
    if (on[SIDE_EDIT] && !rec.empty()) {
      const BamFields F = bam_fields(al.dist, rec, names, off, text);
      if (pile || vcf || mods || depth || errprof) {
        const std::vector<uint8_t> use = pileup_use(F.flag, al.dist);
        if (errprof) errprof_add_batch(ctx, reads.get(), reference, F, al, use, *errprof);
        if (mods) add_batch<ModCalls>(ctx, reads.get(), reference, F, al, use, min_ml, mods_merge_pairs, *mods);
        if (pile || vcf || depth) iv->add_intervals(use, F.contig, al.first, al.last);
        if (pile) add_batch<PileupCalls>(ctx, reads.get(), reference, F, al, use, min_base_quality, pile_merge_pairs, *pile);
        if (vcf) add_batch<VcfCalls>(ctx, reads.get(), reference, F, al, use, min_base_quality, vcf_merge_pairs, *vcf);
      }
      if (sorted) sorted_run_encode(ctx, reads.get(), reference, F, al, (int64_t)rec.size(), *sorted);
      if (!on[SIDE_BAM]) { reads.reset(); return; }
      mm_bam* b = nullptr;
      ck(ctx, mm_bam_encode(ctx, reads.get(), reference, (int64_t)rec.size(), F.read.data(), F.strand.data(), F.contig.data(), al.dist.data(), al.first.data(),
                            al.op_off.data(), al.ops.data(), F.flag.data(), F.mapq.data(), F.name_off.data(), F.all_names.data(), 0, &b), "BAM records");
      int64_t n_records = 0, raw = 0, bytes = 0;
      mm_bam_sizes(b, &n_records, &raw, &bytes);
      members.resize((size_t)bytes);
      if (bytes) mm_bam_fetch(b, (uint8_t*)&members[0]);
      mm_bam_destroy(b);
    }
    reads.reset();
  }
};

// what a worker of MapRun hands to its writer: the finished text of one batch and what the batch adds to every side file
struct BatchDone {
  size_t file = 0;
  std::vector<std::string> names;
  std::vector<int> lens;
  std::vector<int> clens;                                          // --hpc: the compressed lengths (lens stay raw)
  std::vector<int64_t> off;
  std::string text;
  std::string gz;                                                  // --compress-output: the text as BGZF members
  SideBytes side;                                                  // what the batch adds to every side file (side_files.hpp): lines, or BGZF members
  SortedRun sorted;                                                // --bam-sorted: the batch's sorted run
  std::vector<LineMeta> meta;
  double t_mapq = 0, t_fetch = 0, t_format = 0;
};

}  // namespace
