// One run of `classify` on one mappings file (ClassifyRun): the stages in the order run() calls them, each from the structs the earlier ones left to a
// struct of its own — the lines (mapping_lines.hpp), the tables and the EM problem (classify_tables.hpp), the EM over the devices (em_sharded.hpp), the
// files (classify_outputs.hpp).  What stays here is what touches the devices besides the EM: the mappings file read (a BGZF one inflated on the device),
// the gene-level analysis and the identity filter.
#pragma once
#include "bam_reader.hpp"
#include "classify_outputs.hpp"
#include "em_sharded.hpp"
#include "gene_annot.hpp"
#include "query_reader.hpp"
#include <fcntl.h>
#include <sys/mman.h>
#include <memory>

namespace {

struct ClassifyHooks {
  std::function<void()> leave_now;      // the last file: called once everything is written; the process ends there (may be empty)
  std::function<void()> need_devices;   // called before the first device call: the contexts are created beside the parsing of the file (may be empty)
};

// meta::doEM, fEM.h:466-803
struct ClassifyRun {
  const std::vector<Dev>& devs; const EmReduce reduce; const std::string& mapped; const std::string& db; const ClassifyOpts& opts; const ClassifyHooks& hooks;
  const KeptLines* const kept;                                    // mapDirectly --then-classify: the lines in memory (no file is read)
  const CliSwitches& sw;
  PhaseClock pc{sw.timing};
  const unsigned HW = mm::cpu_budget();                        // CPUs this process may keep busy (cpu_budget.hpp: a container's quota counts, not the 256 the machine shows)
  const unsigned WIDE = std::max(1u, HW - std::max(1u, HW / 8));   // width of the pools that compute flat out: under a CPU quota (16 CPUs' worth of time per 100 ms) sixteen such threads plus
                                                               // whatever else runs use the period up, and every thread of the process is stopped for the rest of it (bench: c1 0.11 -> 0.21 s)
  TextBuf text;                                                   // read_file: the file's text, which M's lines point into
  MappingLines M;                                                 // tokenise / adopt
  ClassifyTables C;                                               // read_tables, per_mapping_fields
  std::unique_ptr<Taxonomy> tax;
  EmResult E; std::unique_ptr<LcaJob> lca_job;                    // em
  BootReplicates boot;                                            // bootstrap
  UnmappedTail tail;                                              // write_outputs

  ClassifyRun(const std::vector<Dev>& devs_, EmReduce reduce_, const std::string& mapped_, const std::string& db_, const ClassifyOpts& opts_, const ClassifyHooks& hooks_,
              const KeptLines* kept_, const CliSwitches& sw_)
      : devs(devs_), reduce(reduce_), mapped(mapped_), db(db_), opts(opts_), hooks(hooks_), kept(kept_), sw(sw_) {}

  // A BGZF mappings file (mapDirectly --compress-output, or any bgzip'd mappings file): the block headers are walked here, the blocks
  // inflated on the device a segment of 1 024 at a time (mm_bgzf_inflate), straight into the buffer tokenise() works on.
  void read_bgzf(const std::string& src) {
    const int fd = ::open(src.c_str(), O_RDONLY);
    struct stat stt;
    if (fd < 0 || fstat(fd, &stt) != 0) die("Cannot open mappings file " + src);
    const size_t FS = (size_t)stt.st_size;
    const uint8_t* const F = (const uint8_t*)mmap(nullptr, FS, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (F == MAP_FAILED) die("Cannot map mappings file " + src);
    const std::string err = "Error reading mappings file " + src + ": ";
    std::vector<int64_t> coff, ooff; std::vector<int32_t> clen;
    size_t total = 0;
    for (size_t at = 0; at < FS;) {
      const size_t bs = bam::bgzf_block_size(F + at, FS - at);
      if (!bs && FS - at >= 18) die(err + "bad magic: no BGZF block at byte " + std::to_string(at));
      if (bs < 26 || at + bs > FS) die(err + "truncated BGZF block at byte " + std::to_string(at));
      const size_t isize = bam::rd32(F + at + bs - 4);
      if (isize > 65536) die(err + "corrupt BGZF block at byte " + std::to_string(at) + " (ISIZE " + std::to_string(isize) + ")");
      coff.push_back((int64_t)at); clen.push_back((int32_t)bs); ooff.push_back((int64_t)total);
      total += isize; at += bs;
    }
    if (coff.empty() || clen.back() != 28 || bam::rd32(F + FS - 4) != 0) std::cerr << "Warning: " << src << " does not end in the BGZF end-of-file block; it is probably truncated" << std::endl;
    text.resize(total);
    if (hooks.need_devices) hooks.need_devices();
    mm_ctx* const ctx = devs[0].ctx;
    const size_t SEG = 1024;
    std::vector<int64_t> rc_off(SEG), ro_off(SEG); std::vector<int32_t> st(SEG);
    for (size_t b0 = 0; b0 < coff.size(); b0 += SEG) {
      const size_t n = std::min(SEG, coff.size() - b0), last = b0 + n - 1;
      for (size_t i = 0; i < n; ++i) { rc_off[i] = coff[b0 + i] - coff[b0]; ro_off[i] = ooff[b0 + i] - ooff[b0]; }
      const int64_t comp = coff[last] + clen[last] - coff[b0], out = (last + 1 < ooff.size() ? ooff[last + 1] : (int64_t)total) - ooff[b0];
      const int rc = mm_bgzf_inflate(ctx, F + coff[b0], comp, rc_off.data(), clen.data() + b0, (int32_t)n, (uint8_t*)text.p + ooff[b0], out, ro_off.data(), st.data());
      if (rc == MM_ERR_DATA) for (size_t i = 0; i < n; ++i) if (st[i] != 0) die(err + bam::bgzf_status_message(st[i], (size_t)coff[b0 + i]));
      if (rc != MM_OK) die(std::string("device inflate of the mappings file failed: ") + mm_last_error(ctx));
    }
    munmap((void*)F, FS);
  }
  // `mapped` if it exists (plain text, or BGZF by content), else `mapped`.gz
  void read_file() {
    struct stat probe;
    const std::string src = stat(mapped.c_str(), &probe) == 0 ? mapped : stat((mapped + ".gz").c_str(), &probe) == 0 ? mapped + ".gz" : mapped;
    if (bam::is_bgzf_file(src)) { read_bgzf(src); return; }
    if (is_plain_gzip_file(src)) die("Mappings file " + src + " is plain gzip without BGZF blocks: recompress it with bgzip, or decompress it");
    const int fd = ::open(src.c_str(), O_RDONLY);
    if (fd < 0) die("Cannot open mappings file " + mapped);
    struct stat stt; if (fstat(fd, &stt) != 0) die("Cannot open mappings file " + mapped);
    text.resize((size_t)stt.st_size);
    const size_t PIECE = (size_t)32 << 20, np = (text.size() + PIECE - 1) / PIECE;
    std::atomic<size_t> nx{0}; std::atomic<bool> bad{false};
    on_each_caller_first(std::min<unsigned>({8u, HW, (unsigned)std::max<size_t>(np, 1)}), [&](size_t) {
      for (;;) {
        const size_t i = nx.fetch_add(1); if (i >= np) return;
        size_t a0 = i * PIECE; const size_t e0 = std::min(text.size(), a0 + PIECE);
        while (a0 < e0) { const ssize_t g = pread(fd, &text[a0], e0 - a0, (off_t)a0); if (g <= 0) { bad = true; return; } a0 += (size_t)g; }
      }
    });
    ::close(fd);
    if (bad) die("Cannot read mappings file " + mapped);
  }
  void em() {
    const size_t NT = C.taxa.size();
    E.f.assign(NT, 1 / (double)NT);
    E.post.assign(C.taxon.size(), 0.0); E.best.assign(M.NRD, 0);
    std::cout << "Starting EM..." << std::endl;
    if (hooks.need_devices) hooks.need_devices();
    if (opts.lca.on) lca_job = std::make_unique<LcaJob>(*tax, C.taxa, opts.lca.tau, M.NRD);
    run_em_sharded(devs, reduce, M.off, C.taxon, C.mapq, C.inv, NT, E.f, E.post, E.best, lca_job.get(), sw);
  }
  // --genes: the best mappings of all reads against the annotated genes of their contigs, on the first device (mm_gene_overlap; medians do not merge
  // across shards, and the job is small); PREFIX.EM.geneLevelAnalysis and PREFIX.EM.proteins.TYPE beside the WIMP
  void gene_analysis() {
    const size_t NRD = M.NRD; const std::vector<std::string>& contig_id = M.contig_id;
    std::unordered_map<std::string, int> relevant;                // contigs with a best mapping, in the order of their first one
    std::vector<int> rel_of(contig_id.size(), -1);
    std::vector<int32_t> mc(NRD), ms(NRD), me(NRD); std::vector<double> mi(NRD);
    for (size_t r = 0; r < NRD; ++r) {
      const MapLine& B = M.lines[(size_t)E.best[r]];
      int& k = rel_of[(size_t)B.contig];
      if (k < 0) { k = (int)relevant.size(); relevant.emplace(contig_id[(size_t)B.contig], k); }
      if (B.start > (size_t)INT32_MAX || B.stop > (size_t)INT32_MAX) die("--genes: a mapping of " + contig_id[(size_t)B.contig] + " lies beyond position 2^31");
      mc[r] = k; ms[r] = (int32_t)B.start; me[r] = (int32_t)B.stop; mi[r] = B.ident;
    }
    gene::Annotations A; gene::Results R;
    try { gene::read_annotations(gene::annotations_path(db), relevant, relevant.size(), A); gene::read_proteins(gene::proteins_path(db), A); }
    catch (const gene::Error& e) { die(std::string("--genes: ") + e.what()); }
    std::cout << "Gene-level analysis: found " << relevant.size() << " relevant contig IDs, of which we have annotations for " << A.n_contigs_annotated << "." << std::endl;
    if (A.n_proteins_absent) {
      char pct[32]; snprintf(pct, sizeof pct, "%.2f", 100.0 * (double)A.n_proteins_absent / (double)A.n_protein_lines);
      std::cout << "Warning: " << pct << "% of a total of " << A.n_protein_lines << " in the protein annotations are not in the genome annotations." << std::endl;
    }
    R.group_reads.assign(A.groups.size(), 0); R.group_median.assign(A.groups.size(), 0.0); R.feat_reads.assign(A.feat_name.size(), 0);
    mm_ctx* const ctx = devs[0].ctx;
    ck(ctx, mm_gene_overlap(ctx, (int32_t)relevant.size(), A.contig_gene_off.data(), A.start.data(), A.stop.data(), A.group.data(), (int32_t)A.groups.size(),
                            A.group_feat_off.data(), A.group_feat.data(), (int32_t)A.feat_name.size(), (int64_t)NRD, mc.data(), ms.data(), me.data(), mi.data(),
                            R.group_reads.data(), R.group_median.data(), R.feat_reads.data(), &R.maps_on_annotated), "gene-level analysis");
    std::cout << "Of " << NRD << " mapped reads, " << R.maps_on_annotated << " go to contigs with annotations and " << ((int64_t)NRD - R.maps_on_annotated) << " to contigs without." << std::endl;
    size_t n_genes = 0, n_prot = 0, n_annot = 0;
    gene::found_counts(A, R, &n_genes, &n_prot, &n_annot);
    std::cout << "Found " << n_genes << " genes and " << n_prot << " proteins, of which " << n_annot << " carry any type of additional annotation." << std::endl;
    try {
      gene::write_gene_table(mapped + ".EM.geneLevelAnalysis", A, R);
      const std::vector<std::string> written = gene::write_protein_tables(mapped + ".EM", A, R, NRD);
      for (int t = 0; t < gene::N_TYPES; ++t) {                   // (a table an earlier run left and this one does not have)
        const std::string fn = mapped + ".EM.proteins." + gene::type_name(t);
        if (std::find(written.begin(), written.end(), fn) == written.end()) ::remove(fn.c_str());
      }
      std::cout << "Produced " << mapped << ".EM.geneLevelAnalysis";
      for (const std::string& fn : written) std::cout << ", " << fn;
      std::cout << std::endl;
    } catch (const gene::Error& e) { die(std::string("--genes: ") + e.what()); }
  }
  // --min-identity T: the genomes whose best mappings have a median identity below 100 T are removed, on the first device for all reads (mm_ident_filter;
  // medians do not merge across shards); the files: write_identity_filtered
  void identity_filter(const ClassifyView& V) {
    identf::Filter F;
    F.thr = opts.ident.T * 100.0;                                  // (the script's $identityThreshold *= 100)
    const size_t NT = C.taxa.size(), NE = M.lines.size(), NRD = M.NRD;
    F.ident.resize(NE);
    for (size_t i = 0; i < NE; ++i) F.ident[i] = identf::identity_value(M.lines[i].p, M.lines[i].last_space);
    F.sorted_max.resize(NRD); F.taxon_reads.resize(NT); F.taxon_median.resize(NT); F.taxon_removed.resize(NT); F.read_removed.resize(NRD);
    const bool rf = opts.ident.refit;
    if (rf) { F.read_src.resize(NRD); F.entry_src.resize(NE); F.read_off_out.resize(NRD + 1); }
    mm_ctx* const ctx = devs[0].ctx;
    ck(ctx, mm_ident_filter(ctx, (int64_t)NRD, M.off.data(), C.taxon.data(), F.ident.data(), E.best.data(), (int32_t)NT, F.thr, F.sorted_max.data(), &F.n_with, &F.n_le,
                            F.taxon_reads.data(), F.taxon_median.data(), F.taxon_removed.data(), F.read_removed.data(), rf ? F.read_src.data() : nullptr,
                            rf ? F.entry_src.data() : nullptr, rf ? F.read_off_out.data() : nullptr, rf ? &F.n_reads_out : nullptr, rf ? &F.n_entries_out : nullptr),
       "identity filter");
    F.sorted_max.resize((size_t)F.n_with);
    write_identity_filtered(V, F, tail);
    if (rf) identity_refit(V, F);
  }
  // --refit: the EM again on the mappings of the genomes that stay, from the flat start of em() and over the same devices; the files: write_refit
  void identity_refit(const ClassifyView& V, identf::Filter& F) {
    const size_t NT = C.taxa.size(), NR2 = (size_t)F.n_reads_out, NE2 = (size_t)F.n_entries_out;
    F.read_src.resize(NR2); F.entry_src.resize(NE2); F.read_off_out.resize(NR2 + 1);
    std::vector<int32_t> tx(NE2); std::vector<double> mq(NE2), iv(NE2);
    for (size_t k = 0; k < NE2; ++k) { const size_t e = (size_t)F.entry_src[k]; tx[k] = C.taxon[e]; mq[k] = C.mapq[e]; iv[k] = C.inv[e]; }
    EmResult E2{std::vector<double>(NT, 1 / (double)NT), std::vector<double>(NE2, 0.0), std::vector<int64_t>(NR2, 0)};
    long long rounds = 0;
    if (NR2 > 0) {
      std::cout << "Starting EM on the filtered mappings..." << std::endl;
      if (reduce == EmReduce::Rccl) for (auto& d : devs) mm_comm_destroy(d.ctx);   // (run_em_sharded sets the communicator up)
      run_em_sharded(devs, reduce, F.read_off_out, tx, mq, iv, NT, E2.f, E2.post, E2.best, nullptr, sw, &rounds);
    }
    write_refit(V, F, tx, E2, tail, rounds);
  }
  void write_outputs() {
    const ClassifyView V{mapped, db, M, C, E, *tax};
    std::cout << "Outputting mappings with adjusted alignment qualities." << std::endl;
    PerReadFiles files(mapped);
    Tallies Y;
    std::thread side_files; bool unknown_written = true;
    JoinOnExit side_join{side_files};
    {
      const std::vector<PerReadText> outs = format_and_tally(V, piece_count((size_t)sw.classify_threads, WIDE, M.lines.size(), 50000), HW, Y);
      pc.lap("c5a format");
      // the two side files only read the tallies, which are complete here: they are written beside the per-read files and the WIMP (0.1 s of their own)
      side_files = std::thread([&] {
        std::thread cov_thread([&] { Y.coverage.write(mapped + ".EM.contigCoverage", *tax); });
        unknown_written = write_unknown_species(mapped + ".EM.evidenceUnknownSpecies", db, *tax, Y.coverage, Y.identsPerTaxon, Y.maxReadLen, opts.minReadsU);
        cov_thread.join();
      });
      files.put(outs);
    }
    tail = unmapped_tail(mapped);
    files.r2t << tail.r2t; files.kr << tail.krona;
    const std::map<std::string, double> fmap = cleaned_frequencies(C.taxa, E.f, Y.readsPer, C.st.at("ReadsMapped"));
    pc.lap("c5 output files");
    write_wimp(mapped + ".EM.WIMP", *tax, fmap, Y.readsPer, C.nTotal, C.nUnmapped, C.nTooShort);
    pc.lap("c6 WIMP");
    if (opts.boot.B > 0) { write_bootstrap(mapped + ".EM.WIMP.bootstrap", V, boot.pres, boot.f, boot.empty, fmap, Y.readsPer); pc.lap("c6b WIMP bootstrap"); }
    if (opts.lca.on) {
      write_lca_reads(mapped + ".EM.reads2Taxon.lca", V, *lca_job); write_kreport(mapped + ".EM.kreport", *tax, *lca_job, C.nTotal, C.nUnmapped + C.nTooShort);
      pc.lap("c6c LCA files");
    }
    if (opts.genes.on) { gene_analysis(); pc.lap("c6d gene-level analysis"); }
    if (opts.ident.on) { identity_filter(V); pc.lap("c6e identity filter"); }
    side_files.join();
    if (!unknown_written)
      std::cerr << "Warning: " << db << "/contigNstats_windowSize_1000.txt not found - " << mapped << ".EM.evidenceUnknownSpecies is not written." << std::endl;
    pc.lap("c8 evidence of unknown species + contig coverage");
    if (hooks.leave_now && !sw.full_teardown) { files.close(); pc.report(); hooks.leave_now(); finish_fast(); }   // (a GB of vectors and strings: nothing left to do with them)
  }
  int run() {
    if (kept) M = adopt(*kept);
    else { read_file(); M = tokenise(text.c_str(), text.size(), piece_count((size_t)sw.classify_threads, WIDE, text.size(), (size_t)4 << 20), mapped); }
    C = read_tables(M, mapped, db);
    pc.lap("c1 read mappings + taxonInfo");
    tax = std::make_unique<Taxonomy>(db + "/taxonomy");
    pc.lap("c2 taxonomy");
    per_mapping_fields(M, C);
    pc.lap("c3 per-mapping fields");
    em();
    pc.lap("c4 EM");
    if (opts.boot.B > 0) boot = run_bootstrap(devs, opts.boot, M, C, E.f);
    pc.lap("c4b EM bootstrap");
    write_outputs();
    return 0;
  }
};

int classify_one(const std::vector<Dev>& devs, EmReduce reduce, const std::string& mapped, const std::string& db, const ClassifyOpts& opts, const ClassifyHooks& hooks,
                 const KeptLines* kept, const CliSwitches& sw) {
  return ClassifyRun(devs, reduce, mapped, db, opts, hooks, kept, sw).run();
}

}  // namespace
