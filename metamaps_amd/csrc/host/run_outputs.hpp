// What runs after the last batch of mapDirectly, on the first device: the writers of the outputs that keep a table per query file, and RunOutputs, the owner of everything
// the run's outputs keep between its batches.
#pragma once
#include "batch_outputs.hpp"

namespace {

void write_or_die(const std::string& path, const std::string& text) {
  FILE* out = fopen(path.c_str(), "wb");
  if (!out || fwrite(text.data(), 1, text.size(), out) != text.size() || fclose(out) != 0) die("Error writing " + path);
}
// --pileup, after the last batch of a query file: one merge, one mm_pileup_finish against the reference of `ctx`, and PREFIX.pileup and PREFIX.pileup.contigs
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
// --mods, after the last batch of a query file: one merge, one mm_mod_finish against the reference of `ctx`, and PREFIX.bedmethyl
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
// key, one mm_mod_motifs per group on `ctx`, and PREFIX.motifs.bedmethyl and PREFIX.motifs.tsv
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
// --vcf, after the last batch of a query file and the merge of its rows: one mm_vcf_finish against the reference of `ctx` over the file's intervals, and PREFIX.vcf
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
// a group cut out by key, one mm_consensus per group on `ctx`, and PREFIX.consensus.fa and PREFIX.consensus.tsv appended to as the groups come
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
// --depth, after the last batch of a query file: one mm_depth_profile on `ctx` over the file's intervals and the contigs' lengths, and PREFIX.depth.bedgraph,
// PREFIX.depth.windows and PREFIX.depth.contigs
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
// --error-profile, after the last batch of a query file: one mm_errprof_finish on `ctx` over the file's keys and columns, and PREFIX.errorProfile.substitutions,
// .indels, .qualities and .contigs
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

// Everything the outputs of a run keep between its batches, and what is written from it after the last one.  The plan says which of it is in use.
struct RunOutputs {
  const OutputPlan& plan; const CliSwitches& sw;
  std::deque<FileAcc> files;                                     // one per query file, under plan.per_file_state()
  std::deque<SortedFile> sorted;                                 // --bam-sorted: the runs of every query file (bam_sort_out.hpp)
  std::string bam_head;                                          // --bam: what every PREFIX.bam starts with, its header as BGZF members (the contigs are the run's)
  ContigHits hits;                                               // --extract-taxa, --deplete-taxa: which contigs the lists take

  RunOutputs(const OutputPlan& plan_, const CliSwitches& sw_, size_t n_files) : plan(plan_), sw(sw_) {
    if (plan.per_file_state()) files.resize(n_files);
    if (plan.bam_sorted) sorted.resize(n_files);
  }
  // once the reference's contigs are known, before anything is indexed or mapped: a contig without a taxon under a taxon flag and one too long for a BAI end the run here
  void check_contigs(const std::vector<std::string>& cname, const std::vector<int>& clen) {
    if (plan.reads.any()) hits = contig_hits(plan.reads, cname);
    if (plan.bam_sorted) sorted_bam_check_contigs(cname, clen);
  }
  void deflate_bam_header(mm_ctx* ctx, const std::vector<std::string>& cname, const std::vector<int>& clen) {
    if (plan.side[SIDE_BAM]) bgzf_members(ctx, bam_header(cname, clen), bam_head, "deflate the BAM header");
  }
  // the side outputs of one batch of query file `file`, bound to that file's accumulators and to the batch's sorted run: one alignment for all of them
  BatchSideOutputs batch(size_t file, BatchDone& dn) { return BatchSideOutputs{plan, sw, files.empty() ? nullptr : &files[file], plan.bam_sorted ? &dn.sorted : nullptr, hits}; }
  // the writer, in batch order: the batch's sorted run goes to its query file's temp file
  void append_sorted(size_t file, const std::string& prefix, BatchDone& dn) { if (plan.bam_sorted) sorted[file].append(prefix, dn.sorted); }

  // after the last batch, on `ctx` (the first device) against its reference: every pileup, every depth profile, every error profile, the modification counts
  // with their motifs, the alleles (merged once, then PREFIX.vcf under --vcf and the consensus under --consensus), then the sorted BAMs
  void write(mm_ctx* ctx, const mm_seqset* reference, const std::vector<std::string>& prefixes, const std::vector<std::string>& cname, const std::vector<int>& clen) {
    for (size_t fi = 0; plan.pileup.on && fi < files.size(); ++fi) pileup_write(ctx, reference, files[fi].pile.rows, files[fi].iv, plan.pileup, prefixes[fi], cname, clen);
    for (size_t fi = 0; plan.depth.on && fi < files.size(); ++fi) depth_write(ctx, files[fi].iv, plan.depth, prefixes[fi], cname, clen);
    for (size_t fi = 0; plan.errprof && fi < files.size(); ++fi) errprof_write(ctx, files[fi].errprof, prefixes[fi], cname, clen);
    for (size_t fi = 0; plan.mods.on && fi < files.size(); ++fi) {
      mods_write(ctx, reference, files[fi].mods.rows, plan.mods, prefixes[fi], cname);
      if (plan.motifs.on) motifs_write(ctx, reference, files[fi].mods.rows, plan.mods, plan.motifs, sw.motif_group_bases, prefixes[fi], cname, clen);
    }
    for (size_t fi = 0; plan.vcf_table() && fi < files.size(); ++fi) {
      merge_rows<VcfCalls>(ctx, files[fi].vcf.rows);
      if (plan.vcf.on) vcf_write(ctx, reference, files[fi].vcf.rows, files[fi].iv, plan.vcf, plan.qual.min_base_quality, prefixes[fi], cname, clen);
      if (plan.cons.on) consensus_write(ctx, reference, files[fi].vcf.rows, files[fi].iv, plan.cons, sw.cons_group_bases, prefixes[fi], cname, clen);
    }
    if (plan.bam_sorted) {
      std::string head;
      bgzf_members(ctx, bam_header(cname, clen, true), head, "deflate the sorted BAM header");
      for (size_t fi = 0; fi < sorted.size(); ++fi) sorted_bam_write(ctx, sorted[fi], prefixes[fi], head, clen, sw.bam_sort_window);
    }
  }
};

}  // namespace
