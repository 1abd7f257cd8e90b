// One run of mapDirectly / index / mapAgainstIndex (MapRun).  What it stands on: the reference loader (ref_loader.hpp), the formatter of the
// mapping lines (map_format.hpp) and the run's outputs beside PREFIX (output_plan.hpp says which; run_outputs.hpp and batch_outputs.hpp make them).
#pragma once
#include "classify_run.hpp"
#include "cli_device.hpp"
#include "cli_switches.hpp"
#include "id_set.hpp"
#include "index_files.hpp"
#include "map_format.hpp"
#include "query_reader.hpp"
#include "ref_loader.hpp"
#include "run_outputs.hpp"
#include <climits>
#include <cmath>
#include <fstream>
#include <optional>
#include <sstream>

namespace {

// ------------------------------------------------------------------------------------------------------
// mapDirectly, index and mapAgainstIndex share everything but where the reference comes from:
//   index            FASTA -> chunk plan -> PREFIX.N.seqset per chunk (+ PREFIX.index / .arguments / .contigs)   mapWrap.h:358-405
//   mapAgainstIndex  those files -> device indexes -> map                                                         mapWrap.h:443-554
//   mapDirectly      FASTA -> chunk plan -> device indexes -> map                                                 mapWrap.h:407-441
// The stored form is the packed reference, not the reference's Boost archive of the sketch: rebuilding the device
// index takes seconds and the file stays a third of the FASTA's size.
//
// Several GPUs (--gpus N; the reference's -t N worker pool, computeMap.hpp:104-176, becomes one context per device):
//   replicated   every device holds every chunk index; read batches go to whichever worker is free and the output is written
//                in batch order (= input order, all ThreadPool.hpp:13-17 guarantees).  No exchange between devices.
//   sharded      (--shard-index, or automatic when the chunk indexes fit the devices together but not one of them) chunk c
//                lives on device c mod N, every read batch visits every device, the records stay on the device that made them
//                and go to the batch's owner device — RCCL send / receive between physical devices (mm_mapping_gather), device-to-
//                device copies between logical devices of one GPU (mm_mapping_concat), through the host only with --host-gather —
//                for the merge in chunk order and the mapping qualities: what the reference does with its PREFIX.N files
//                (mapWrap.h:417-437, :128-145).
//   streamed     (--stream-chunks, or automatic when not even that fits) rounds of N chunks, one per device, built, mapped
//                against every (device-resident) read batch and dropped.

// One run of mapDirectly / index / mapAgainstIndex.  The state every stage shares lives in the object; the stages are its methods, in the order run()
// calls them: parameters -> devices -> reference (parsed, packed, uploaded) or stored index -> chunk plan -> placement of the chunk indexes
// (replicated / sharded / streamed) -> read batches through the worker pipeline (replicated) or chunk-major rounds with the exchange of the
// records (sharded / streamed) -> writers -> optionally classify in-process.  (Until round 5 this was one 800-line function.)
struct MapRun {
  const Options& o; const CliSwitches& sw; const std::string mode;
  // what the command line asks for beside PREFIX (output_plan.hpp).  With an aligned output (plan.edit()) the packed reference stays on every device; a batch's
  // reads live as long as the plan says (keep_reads(), reads_until_text()).  The read files need no alignment and no resident reference.
  const OutputPlan& plan;
  std::optional<RunOutputs> outs;                                // what the outputs keep between the batches (run_outputs.hpp): made once the number of query files is known
  const bool from_index, only_index;
  std::string ref; uint64_t refSize = 0, maxMem = 0; int k = 16, w = 0, minLen = 1000; double pval = 1e-3; float pi = 80;
  std::string ipre;
  std::vector<std::string> queries, prefixes;
  PhaseClock pc{sw.timing};
  std::vector<Dev> devs; size_t G = 0; mm_ctx* ctx0 = nullptr;
  std::vector<std::string> cname; std::vector<int> clen;
  // --hpc: the sequences are homopolymer-compressed on the device (mm_seqset_hpc) and everything from the chunk plan to the mapping qualities sees the
  // compressed ones: clen holds the compressed contig lengths, clen_raw what is printed; hpc_map[d] translates the records' coordinates on device d
  const bool hpc = o.v.count("hpc") != 0;
  std::vector<int> clen_raw; std::vector<mm_hpc_map*> hpc_map;
  using Chunk = IndexChunk;                                      // (index_files.hpp)
  std::vector<Chunk> chunks;
  // The packed reference (2 bits per base + exception runs, a quarter of the FASTA's size) lives on every device that builds indexes
  // from it; the host holds contig names and lengths only.  Index chunks are cut out of it on the device (mm_seqset_slice).
  std::vector<mm_seqset*> refset;
  uint64_t hbm_free = 0;
  const int64_t BATCH_READS = sw.batch_reads, BATCH_BASES = sw.batch_bases;   // ~0.25 Gbp per device batch (16 ms of mapping); the next ones are parsed meanwhile
  size_t WPD = 4;                                               // worker contexts per device (replicated mode)
  std::vector<mm_ctx*> wctx;
  uint64_t ref_bases = 0;
  mm_index* whole = nullptr;                                     // index of the whole reference on device 0, when one was built for the chunk plan
  size_t NC = 0;
  enum class Place { Replicated, Sharded, Streamed } place = Place::Replicated;
  std::vector<int> thr_of;
  std::map<int64_t, int64_t> thr_acc; int thr = INT_MAX;          // occurrence histogram accumulated over the chunks, never cleared (winSketch.hpp:452-494)
  mm_map_params mp{};
  std::vector<int32_t> chunk_base;
  using Done = BatchDone;                                        // what a worker hands to the writer (batch_outputs.hpp)
  // --then-classify: the batches of every query file as they were written, in order (text + the parsed fields of every line): what classify takes
  // instead of the file
  const bool keep_lines = o.v.count("then-classify") && !sw.classify_from_file;
  // --compress-output: the mappings go to PREFIX.gz as BGZF; a batch's text is deflated by the context that mapped it, right behind its formatting
  const bool compress = o.v.count("compress-output") != 0;
  std::vector<std::vector<std::unique_ptr<Done>>> kept;
  // the writer: batches in input order -> PREFIX, .meta.unmappedReadsLengths, .meta, .parameters of every query file (mapWrap.h:34-213)
  struct Writer {
    std::mutex m; std::condition_variable cv; std::map<size_t, std::unique_ptr<Done>> ready;
    void put(size_t seq, std::unique_ptr<Done> d) { std::lock_guard<std::mutex> lk(m); ready[seq] = std::move(d); cv.notify_all(); }
  } writer;
  Reader reader;                                                 // the reader thread's queue (query_reader.hpp): `take` hands the batches out in order
  std::deque<MappedFile> mapped;                                 // query files whose sequences the batches point into: alive until the end
  std::thread prewarm;                                           // (declared last: joined first)

  MapRun(const Options& o_, const std::string& mode_, const CliSwitches& sw_, const OutputPlan& plan_)
      : o(o_), sw(sw_), mode(mode_), plan(plan_), from_index(mode_ == "mapAgainstIndex"), only_index(mode_ == "index") {}
  ~MapRun() { if (prewarm.joinable()) prewarm.join(); }

  void read_parameters() {
    if (hpc && mode != "mapDirectly") die("--hpc belongs to mapDirectly: " + mode + " --hpc (stored indexes of compressed sequences) is not provided");
    if (!from_index && !o.v.count("reference")) die("Provide reference file (s)");
    if ((from_index || only_index) && !o.v.count("index")) die("Please provide index");
    if (!only_index && !o.v.count("query")) die("Provide query file (s)");
    if (!only_index && !o.v.count("output")) die("Provide output file");
    ipre = o.v.count("index") ? o.v.at("index") : "";
    if (!from_index) {
      ref = o.v.at("reference");
      refSize = file_size(ref);
      maxMem = o.v.count("maxmemory") ? (uint64_t)(std::pow(1024, 3) * std::stoull(o.v.at("maxmemory"))) : 0;
      if (o.v.count("maxmemory-bytes")) maxMem = std::stoull(o.v.at("maxmemory-bytes"));
      k = o.v.count("kmer") ? std::stoi(o.v.at("kmer")) : 16;
      pval = o.v.count("pval") ? std::stod(o.v.at("pval")) : 1e-3;
      minLen = o.v.count("minReadLen") ? std::stoi(o.v.at("minReadLen")) : 1000;
      pi = o.v.count("perc_identity") ? std::stof(o.v.at("perc_identity")) : 80;
      if (o.v.count("window")) {                                   // parseCmdArgs.hpp:363-374
        w = std::stoi(o.v.at("window"));
        pval = mm_estimate_pvalue(minLen * 2 / w, k, pi, minLen, refSize);
      } else w = mm_recommended_window(pval, k, pi, minLen, refSize);
    } else {                                                       // the parameters travel with the index (mapWrap.h:447-461)
      const IndexArguments a = read_index_arguments(ipre);
      k = a.k; w = a.w; minLen = a.minLen; pi = a.pi; pval = a.pval; refSize = a.refSize; maxMem = a.maxMem; ref = a.ref;
    }
    if (!only_index) {
      queries = split(o.v.at("query"), ","); prefixes = split(o.v.at("output"), ",");
      if (queries.size() != prefixes.size()) die("Please specify an equal number of input and output files (as comma-separated lists)");
    }
  }

  void open_devices() {
    for (int p : device_list(o)) { Dev d; d.phys = p; devs.push_back(d); }
    if (only_index) devs.resize(1);
    G = devs.size();
    for (auto& d : devs) if (mm_ctx_create(d.phys, &d.ctx) != MM_OK) die("No MI355X (gfx950) device available — this build has no CPU path");
    ctx0 = devs[0].ctx;
    pc.lap("0 context");
    refset.assign(G, nullptr);
    query_free();
    // ---- reads (computeMap.hpp:104-172 + unifyFiles mapWrap.h:34-213)
    reader.max_queued = std::max<size_t>(2, 2 * G);
    // worker contexts of the replicated mode (WPD per device, --workers-per-gpu).  The ones beside the device's first context come up while the
    // index is built, each with its upload staging in place (a batch-sized dummy goes through mm_seqset_upload once: pinned buffer, device
    // block): the first batch of a worker used to spend 40-60 ms there, and 38 ms creating its stream, with the device idle.
    WPD = o.v.count("workers-per-gpu") ? (size_t)std::max(1, std::stoi(o.v.at("workers-per-gpu")))
        : sw.workers;
    wctx.assign(G * WPD, nullptr);
  }

  void query_free() {
    char nm[8]; int cus; uint64_t tot; mm_ctx_device_info(ctx0, nm, sizeof nm, &cus, &tot, &hbm_free);
    size_t share = 0; for (auto& d : devs) share += d.phys == devs[0].phys;   // logical devices of one physical device (--devices 0,0,..) share its memory
    hbm_free /= std::max<size_t>(share, 1);
  }

  // Resident bytes of the index of `bases` reference bases: N = 2 bases / (w + 1) entries; U distinct hashes — minimizer
  // hashes are window minima, so they crowd into the low end of the 32-bit space: measured 5.92e8 distinct among 5.94e9 entries at w = 8,
  // i.e. an effective space of H = 1.3 * 2^32 / (w + 1) values that fills as U = H (1 - exp(-N / H)); pos 8 N + occurrence lists padded to
  // 64-byte sectors 8 (N + 7 U) at most + a quarter of that in bin codes + 29 U of table.  Per base this FALLS with the size of the
  // reference: 6 bytes at 26.8 Gbp, 22 at 1 Gbp, where nearly every hash is a list of one padded to eight (a flat 5.5 bytes per base,
  // rounds 1-3, let a 0.5 Gbp planning range ask for 5.5 GiB on a device with 2 GiB left — found with MM_DEVICE_BYTES_CAP).  The build
  // holds another 12 N of sort buffers at its peak.
  double index_bytes(uint64_t bases, bool peak) const {
    const double N = 2.0 * (double)bases / (double)(w + 1), H = 1.3 * 4294967296.0 / (double)(w + 1), U = H * (1 - std::exp(-N / H));
    return 18.0 * N + 99.0 * U + (peak ? 12.0 * N : 0.0);
  }
  // `share` of the index of `bases` bases fits beside what the device already holds (the estimate errs on the large side by ~10 %)
  bool fits(uint64_t bases, double share) const { return index_bytes(bases, share >= 1.0) * share <= 0.8 * (double)hbm_free; }
  mm_seqset* make_part(size_t d, int a, int bnd) {               // contigs [a, bnd) of the reference as a set of their own, on device d
    mm_seqset* part; ck(devs[d].ctx, mm_seqset_slice(devs[d].ctx, refset[d], a, bnd - a, &part), "reference chunk");
    return part;
  }
  void drop_refsets() { for (auto*& r : refset) if (r) { mm_seqset_destroy(r); r = nullptr; } }

  // (started as soon as the reference has been parsed: the first batches are ready when the index is)
  void start_reader() { if (reader.th.joinable() || reader.started) return; reader.started = true; 
    reader.th = std::thread([this]() { QueryReader(reader, queries, BATCH_READS, BATCH_BASES, devs[0].phys, pc, mapped, sw, plan.qual.keep, plan.mods.on ? &plan.mods : nullptr).run(); }); }
  void start_prewarm() {
    if (prewarm.joinable() || sw.no_prewarm) return;
    int64_t query_bytes = 0; for (auto& q : queries) query_bytes += (int64_t)file_size(q);
    const int64_t warm_bases = std::min<int64_t>(BATCH_BASES, query_bytes / 2);   // (a FASTQ is two bytes per base; small inputs get small staging)
    prewarm = std::thread([&, warm_bases]() {
      static const std::string dummy((size_t)1 << 20, 'A');
      std::vector<std::thread> th;
      for (size_t d = 0; d < G; ++d) for (size_t wi = 1; wi < WPD; ++wi) th.emplace_back([&, d, wi]() {
        mm_ctx* c = nullptr;
        if (mm_ctx_create(devs[d].phys, &c) != MM_OK) die("cannot create a worker context");
        mm_seqset* sq = nullptr;
        if (mm_seqset_create(c, &sq) == MM_OK) {                  // (a failure here only means the first batch pays for its staging itself)
          bool ok = true;
          for (int64_t b = 0; ok && b < warm_bases; b += (int64_t)dummy.size()) ok = mm_seqset_add_view(sq, dummy.data(), (int64_t)dummy.size()) == MM_OK;
          if (ok) (void)mm_seqset_upload(sq);
          mm_seqset_destroy(sq);
        }
        wctx[d * WPD + wi] = c;
      });
      for (auto& t : th) t.join();
    });
  }

  // ---- reference (winSketch.hpp:180-365): parsed, packed and uploaded to every device that builds indexes from it
  void load_reference() {
    ReferenceLoader loader(sw, devs, only_index ? 1 : G, pc, cname, clen, ref_bases);
    loader.load(ref, refset);
    pc.lap("1 reference parse + pack + upload");
    pc.add("2 reference pack+upload (inside 1)", loader.t_pack);
    outs->check_contigs(cname, clen);                            // (before anything is indexed or mapped)
    if (hpc) compress_reference();
    if (!only_index) { if (!sw.late_reader) start_reader(); start_prewarm(); }   // (MM_CLI_LATE_READER: measurement aid — the reader starts when the index is built)
    // the packed reference now lives on the device (0.25 B per base, for as long as chunks are cut out of it): what is left is what the indexes get
    query_free();
  }

  // --hpc: the reference of every device compressed where it lies, once, before the chunk plan; the raw packed set goes, the map stays
  void compress_reference() {
    hpc_map.assign(refset.size(), nullptr);
    std::vector<int32_t> cl(cname.size());
    on_each(refset.size(), [&](size_t d) {
      if (!refset[d]) return;
      mm_seqset* c = nullptr;
      ck(devs[d].ctx, mm_seqset_hpc(devs[d].ctx, refset[d], &c, &hpc_map[d]), "homopolymer compression of the reference");
      mm_seqset_destroy(refset[d]); refset[d] = c;
      if (d == 0 && !cl.empty()) ck(devs[d].ctx, mm_seqset_lengths(c, cl.data()), "compressed contig lengths");
    });
    clen_raw = clen; ref_bases = 0;
    for (size_t i = 0; i < clen.size(); ++i) { clen[i] = cl[i]; ref_bases += (uint64_t)cl[i]; }
    std::cout << "INFO, --hpc: " << ref_bases << " reference bases after homopolymer compression, coordinate map of " << (mm_hpc_map_device_bytes(hpc_map[0]) >> 10) << " KiB per device\n";
    pc.lap("2h reference homopolymer compression");
  }

  // ---- the chunk plan of --maxmemory (winSketch.hpp:274-329): on the index of the whole reference when that fits, on contig ranges otherwise
  void plan_chunks() {
  std::vector<int32_t> first(1, 0);
  if (!maxMem || fits(ref_bases, 1.0)) {
    // the index of the whole reference: the only chunk, or what the chunk rule of --maxmemory is evaluated on
    if (!maxMem && o.stream) die("--stream-chunks needs --maxmemory (the chunk rule of the reference, winSketch.hpp:274-329)");
    mm_seqset* contigs = refset[0];
    ck(ctx0, mm_index_build(ctx0, contigs, k, w, &whole), "index");
    pc.lap("3 index build");
    if (maxMem) {
      int32_t n = 0;
      ck(ctx0, mm_index_plan_chunks(ctx0, whole, maxMem, nullptr, 0, &n), "chunk plan");
      first.resize((size_t)n);
      ck(ctx0, mm_index_plan_chunks(ctx0, whole, maxMem, first.data(), n, &n), "chunk plan");
    }
    if (only_index && first.size() == 1 && !o.v.count("full-index")) ck(ctx0, mm_seqset_save(contigs, (ipre + ".1.seqset").c_str()), "store index chunk");
  } else {
    // The chunk rule without an index of the whole reference: it decides to close a chunk from the chunk's own content
    // and the next contig only, so it can be evaluated on the index of a contig range that fits the device.  Every cut
    // inside the range is final; the range's last chunk is not (it may go on), so the next range starts there.
    std::cout << "INFO, the index of " << ref_bases << " reference bases does not fit one device's " << (hbm_free >> 30) << " GiB: the chunk rule is evaluated on contig ranges\n";
    const int C = (int)cname.size();
    uint64_t range_bases = 0;
    if (o.v.count("stream-range-bases")) range_bases = std::stoull(o.v.at("stream-range-bases"));
    else {                                                     // the largest range whose index BUILD stays within 70 % of what is free
      uint64_t lo = 1, hi = ref_bases;
      while (lo < hi) { const uint64_t mid = lo + (hi - lo + 1) / 2; if (index_bytes(mid, true) <= 0.7 * (double)hbm_free) lo = mid; else hi = mid - 1; }
      range_bases = lo;
    }
    int c0 = 0;
    while (c0 < C) {
      int c1 = c0; uint64_t bases = 0;
      while (c1 < C && (bases < range_bases || c1 == c0)) bases += (uint64_t)clen[(size_t)c1++];
      mm_seqset* part = make_part(0, c0, c1);
      mm_index* ri; ck(ctx0, mm_index_build(ctx0, part, k, w, &ri), "index (chunk planning range)");
      mm_seqset_destroy(part);
      int32_t n = 0;
      ck(ctx0, mm_index_plan_chunks(ctx0, ri, maxMem, nullptr, 0, &n), "chunk plan");
      std::vector<int32_t> loc((size_t)n);
      ck(ctx0, mm_index_plan_chunks(ctx0, ri, maxMem, loc.data(), n, &n), "chunk plan");
      mm_index_destroy(ri);
      if (n == 1 && c1 < C) {                                   // the chunk that starts at c0 is longer than the range
        if (index_bytes(bases * 2, true) > 0.9 * (double)hbm_free && !o.v.count("stream-range-bases"))
          die("--maxmemory describes index chunks larger than this device can hold one at a time");
        range_bases = bases * 2; continue;
      }
      for (int32_t j = 1; j < n; ++j) first.push_back(c0 + loc[(size_t)j]);
      if (c1 == C) break;
      c0 += loc[(size_t)n - 1];
    }
    pc.lap("3 index build");
  }
  for (size_t c = 0; c < first.size(); ++c) {
    const int a = first[c], b = c + 1 < first.size() ? first[c + 1] : (int)cname.size();
    chunks.push_back(Chunk{a, b - a, ""});
  }
  }

  // `metamaps index`: PREFIX.N.seqset (or .mmidx with --full-index) per chunk + PREFIX.index / .arguments / .contigs (mapWrap.h:358-405)
  int write_index_files() {
    write_index_flag(ipre, 0, {});                               // (index_files.hpp: the text files of a stored index)
    std::vector<std::string> chunk_files;
    const bool full = o.v.count("full-index") != 0;            // the device index itself (mm_index_save) instead of the packed reference it is rebuilt from
    for (size_t c = 0; c < chunks.size(); ++c) {
      chunk_files.push_back(ipre + "." + std::to_string(c + 1) + (full ? ".mmidx" : ".seqset"));
      if (full) {
        mm_index* ix = whole;
        if (!(chunks.size() == 1 && whole)) {
          if (whole) { mm_index_destroy(whole); whole = nullptr; }   // (the chunk rule is done with it)
          mm_seqset* part = make_part(0, chunks[c].first, chunks[c].first + chunks[c].count);
          ck(ctx0, mm_index_build(ctx0, part, k, w, &ix), "index chunk");
          mm_seqset_destroy(part);
        }
        ck(ctx0, mm_index_save(ix, chunk_files.back().c_str()), "store index chunk");
        if (ix != whole) mm_index_destroy(ix);
        continue;
      }
      if (chunks.size() == 1 && whole) continue;                // stored above, from the set the index was built on
      mm_seqset* part = make_part(0, chunks[c].first, chunks[c].first + chunks[c].count);
      ck(ctx0, mm_seqset_save(part, chunk_files.back().c_str()), "store index chunk");
      mm_seqset_destroy(part);
    }
    if (whole) mm_index_destroy(whole);
    drop_refsets();
    IndexArguments a;
    a.k = k; a.w = w; a.minLen = minLen; a.pi = pi; a.pval = pval; a.refSize = refSize; a.maxMem = maxMem; a.ref = ref;
    write_index_arguments(ipre, a);
    write_index_contigs(ipre, chunks, cname, clen);
    write_index_flag(ipre, 1, chunk_files);
    mm_ctx_destroy(ctx0);
    return 0;
  }

  // ---- where the chunk indexes live
  void decide_placement() {
    NC = chunks.size();
    if (o.stream) place = Place::Streamed;
    else if (o.shard) place = Place::Sharded;
    else if (NC > 1) {
      // every chunk index resident on every device / chunk c on device c mod G / one round of G chunks at a time: the first that fits
      // (a chunk index costs more per base than the whole reference's: fewer occurrences per hash, the same padding per list)
      std::vector<double> per_dev(G, 0.0); double all = 0, build_extra = 0;
      for (size_t c = 0; c < NC; ++c) {
        uint64_t cb = 0; for (int i = chunks[c].first; i < chunks[c].first + chunks[c].count; ++i) cb += (uint64_t)clen[(size_t)i];
        const double b = index_bytes(cb, false);
        all += b; per_dev[c % G] += b; build_extra = std::max(build_extra, index_bytes(cb, true) - b);
      }
      const double room = 0.8 * (double)hbm_free;
      if (all + build_extra <= room) place = Place::Replicated;
      else place = (G > 1 && *std::max_element(per_dev.begin(), per_dev.end()) + build_extra <= room) ? Place::Sharded : Place::Streamed;
    }
    if (place != Place::Replicated && !o.stream && !o.shard) {
      std::cout << "INFO, the index of " << ref_bases << " reference bases does not fit one device's " << (hbm_free >> 30) << " GiB: "
                << (place == Place::Sharded ? "the chunk indexes are spread over the devices" : "chunk indexes are built and mapped one after the other") << "\n";
    }
    if (place != Place::Replicated && NC == 1 && !from_index && !maxMem) die("--stream-chunks / --shard-index need --maxmemory (the chunk rule of the reference, winSketch.hpp:274-329)");
    if (plan.reads.any() && place != Place::Replicated)
      die(std::string("--") + plan.reads.first_flag() + " needs every chunk index resident on every device, and this index does not fit one: a batch's reads stay on the device only then");
    if (plan.edit() && place != Place::Replicated)
      die(std::string(plan.flag_name()) + " needs the whole reference resident on every device, and this index does not fit one: run without it");
    for (auto& d : devs) d.idx.assign(NC, nullptr);
    thr_of.assign(NC, INT_MAX);
  }

  void build_chunk(Dev& d, size_t c) {                            // the index of chunk c on device d
    const Chunk& ch = chunks[c];
    if (d.idx[c]) return;
    if (whole && NC == 1 && &d == &devs[0]) { d.idx[c] = whole; whole = nullptr; return; }
    mm_seqset* part;
    if (ch.file.size() > 6 && ch.file.compare(ch.file.size() - 6, 6, ".mmidx") == 0) {   // `index --full-index`: the stored device index, nothing to build
      ck(d.ctx, mm_index_load(d.ctx, ch.file.c_str(), &d.idx[c]), "load index chunk");
      mm_index_info info; mm_index_get_info(d.idx[c], &info);
      if ((int64_t)ch.count != info.n_contigs) die("Index chunk " + ch.file + " does not match " + ipre + ".contigs");
      return;
    }
    if (!ch.file.empty()) {
      ck(d.ctx, mm_seqset_load(d.ctx, ch.file.c_str(), &part), "load index chunk");
      if ((int64_t)ch.count != mm_seqset_count(part)) die("Index chunk " + ch.file + " does not match " + ipre + ".contigs");
    } else if (NC == 1) part = refset[(size_t)(&d - &devs[0])];    // the whole reference is the chunk: no copy
    else part = make_part((size_t)(&d - &devs[0]), ch.first, ch.first + ch.count);
    ck(d.ctx, mm_index_build(d.ctx, part, k, w, &d.idx[c]), "index chunk");
    if (!(ch.file.empty() && NC == 1)) mm_seqset_destroy(part);
  }
  // freqThreshold of chunk c from the histogram accumulated over chunks 0..c: call once per chunk, in chunk order, after some
  // device has built it; the value is then set on every copy of that chunk
  void settle_threshold(size_t c) {
    mm_index* any = nullptr;
    for (auto& d : devs) if (d.idx[c]) { any = d.idx[c]; break; }
    int64_t n = 0; mm_index_freq_hist(any, nullptr, nullptr, 0, &n);
    std::vector<int64_t> cc((size_t)n), hh((size_t)n); mm_index_freq_hist(any, cc.data(), hh.data(), n, &n);
    for (int64_t i = 0; i < n; ++i) thr_acc[cc[(size_t)i]] += hh[(size_t)i];
    mm_index_info info; mm_index_get_info(any, &info);
    if (info.n_unique_hashes > 0) {
      std::vector<int64_t> ac, ah; for (auto& kv : thr_acc) { ac.push_back(kv.first); ah.push_back(kv.second); }
      thr = mm_freq_threshold_from_hist(ac.data(), ah.data(), (int64_t)ac.size(), info.n_unique_hashes, thr);
    }
    thr_of[c] = thr;
    for (auto& d : devs) if (d.idx[c]) mm_index_set_freq_threshold(d.idx[c], thr);
    std::cout << "INFO, index chunk " << c + 1 << "/" << NC << ": contigs " << chunks[c].first << ".." << chunks[c].first + chunks[c].count - 1
              << ", " << info.n_entries << " minimizers, " << info.n_unique_hashes << " unique hashes\n";
  }

  // replicated: every chunk index on every device before the first batch; the packed reference goes
  void build_resident_indexes() {
    if (whole && !(NC == 1 && place == Place::Replicated)) { mm_index_destroy(whole); whole = nullptr; }
    if (place == Place::Replicated) {
      on_each(G, [&](size_t d) { for (size_t c = 0; c < NC; ++c) build_chunk(devs[d], c); });
      for (size_t c = 0; c < NC; ++c) settle_threshold(c);
      if (!plan.edit()) drop_refsets();
      pc.lap("3 index build");
    }
  }

  mm_seqset* upload_batch(mm_ctx* ctx, const Batch& bt) {
    mm_seqset* reads; ck(ctx, mm_seqset_create(ctx, &reads), "seqset");
    for (size_t r = 0; r < bt.names.size(); ++r) {
      if (bt.nt16) ck(ctx, mm_seqset_add_nt16(reads, (const uint8_t*)bt.seq_of(r), (int64_t)bt.lens[r], bt.rev[r]), "add read");
      else ck(ctx, mm_seqset_add_view(reads, bt.seq_of(r), (int64_t)bt.lens[r]), "add read");
      if (const char* q = bt.qual_of(r)) ck(ctx, mm_seqset_add_qual(reads, (const uint8_t*)q, (int64_t)bt.lens[r], bt.qual_offset), "add qualities");   // (--base-qualities)
      ck(ctx, bt.add_mods_to(reads, r), "add modifications");    // (--mods: nothing for a read without tags)
    }
    ck(ctx, mm_seqset_upload(reads), "upload reads");
    if (hpc) {                                                     // compressed on the context that maps the batch, between upload and K1
      mm_seqset* c = nullptr;
      ck(ctx, mm_seqset_hpc(ctx, reads, &c, nullptr), "homopolymer compression of the reads");
      mm_seqset_destroy(reads); reads = c;
    }
    return reads;
  }
  std::vector<int> compressed_lengths(mm_ctx* ctx, const mm_seqset* reads) {   // --hpc: what -m, the skips and the mapping qualities count
    std::vector<int> cl((size_t)mm_seqset_count(reads));
    if (!cl.empty()) ck(ctx, mm_seqset_lengths(reads, cl.data()), "compressed read lengths");
    return cl;
  }
  // one "PREFIX.N" per chunk in the reference (mapWrap.h:419-437); `sketch_of`: an earlier mapping of the same batch on this device,
  // whose minimizers and sketches are reused (they do not depend on the index)
  mm_mapping* map_chunk(mm_ctx* ctx, mm_index* idx, mm_seqset* reads, const mm_mapping* sketch_of = nullptr) {
    mm_mapping* pm;
    if (sketch_of) ck(ctx, mm_map_batch_reusing(ctx, idx, reads, &mp, sketch_of, &pm), "map");
    else ck(ctx, mm_map_batch(ctx, idx, reads, &mp, &pm), "map");
    if (!o.all) ck(ctx, mm_mapping_keep_best(ctx, pm, k), "best mappings");
    return pm;
  }
  // mapping qualities + text + side outputs; consumes m (and the reads that the side outputs have kept: none in the sharded and streamed modes)
  std::unique_ptr<Done> finish_mapping(mm_ctx* ctx, size_t dev, mm_mapping* m, std::vector<std::string>&& names, std::vector<int>&& lens,
                                       std::vector<int>&& clens, size_t file, ReadsPtr reads = nullptr) {
    auto dn = std::make_unique<Done>();
    dn->file = file; dn->names = std::move(names); dn->lens = std::move(lens); dn->clens = std::move(clens);
    const auto f0 = std::chrono::steady_clock::now();
    ck(ctx, mm_mapping_add_qualities(ctx, m, nullptr, k), "mapping qualities");
    dn->off.resize(dn->names.size() + 1);
    ck(ctx, mm_mapping_fetch(m, dn->off.data(), nullptr, 0), "fetch");
    std::vector<int64_t> raw_end;
    if (hpc) {                                                     // the records' start -> raw coordinates on the device; field 9 comes back beside them
      raw_end.resize((size_t)dn->off.back());
      ck(ctx, mm_mapping_to_raw(ctx, m, hpc_map[dev], raw_end.data(), (int64_t)raw_end.size()), "raw coordinates");
    }
    const auto f1 = std::chrono::steady_clock::now();
    std::vector<mm_map_record> rec((size_t)dn->off.back());
    ck(ctx, mm_mapping_fetch(m, dn->off.data(), rec.data(), (int64_t)rec.size()), "fetch");
    BatchSideOutputs so = outs->batch(file, *dn);
    so.from_mapping(ctx, m, reads, refset[dev], pi, rec, dn->names, dn->lens, dn->off, cname, clen, dn->side);
    mm_mapping_destroy(m);
    const auto f2 = std::chrono::steady_clock::now();
    format_records(dn->names, dn->lens, dn->off, rec, cname, hpc ? clen_raw : clen, k, dn->text, keep_lines ? &dn->meta : nullptr,
                   hpc ? raw_end.data() : nullptr, sw);
    so.from_text(ctx, reads, refset[dev], rec, dn->names, dn->off, dn->text, dn->side);   // --bam: the mapping qualities come from the formatted lines
    if (compress) deflate_text(ctx, *dn);
    const auto f3 = std::chrono::steady_clock::now();
    pc.add("7a mapping qualities + offsets", std::chrono::duration<double>(f1 - f0).count());
    pc.add("7b fetch records", std::chrono::duration<double>(f2 - f1).count());
    pc.add("7c format", std::chrono::duration<double>(f3 - f2).count());
    dn->t_mapq = std::chrono::duration<double>(f1 - f0).count();
    dn->t_fetch = std::chrono::duration<double>(f2 - f1).count();
    dn->t_format = std::chrono::duration<double>(f3 - f2).count();
    return dn;
  }
  // the text of a batch as BGZF members (batch_outputs.hpp: the batches' members concatenate in output order); the text itself is kept only
  // where --then-classify takes its lines from memory
  void deflate_text(mm_ctx* ctx, Done& dn) {
    const auto z0 = std::chrono::steady_clock::now();
    bgzf_members(ctx, dn.text, dn.gz, "deflate the mappings");
    if (!keep_lines) std::string().swap(dn.text);
    pc.add("7d deflate", std::chrono::duration<double>(std::chrono::steady_clock::now() - z0).count());
  }
  // next(file, seq): batch `seq` if it belongs to that file, nullptr once the file has ended
  void write_all(const std::function<std::unique_ptr<Done>(size_t, size_t)>& next) {
    size_t seq = 0;
    for (size_t fi = 0; fi < queries.size(); ++fi) {
      const std::string& prefix = prefixes[fi];
      if (compress) ::unlink(prefix.c_str());                    // (classify prefers a plain PREFIX: one left from an earlier run must not shadow PREFIX.gz)
      const std::string out_name = compress ? prefix + ".gz" : prefix;
      std::ofstream out(out_name, std::ios::binary), unm(prefix + ".meta.unmappedReadsLengths");
      if (!out.is_open()) die("Cannot open output file " + out_name);
      std::array<std::ofstream, N_SIDE> sf;
      for (size_t s = 0; s < N_SIDE; ++s) if (plan.side[s]) {
        sf[s].open(prefix + side_suffix((int)s, plan.reads.with_qual), std::ios::binary);
        if (!sf[s].is_open()) die("Cannot open output file " + prefix + side_suffix((int)s, plan.reads.with_qual));
        if (kSideFiles[s].head) sf[s].write(outs->bam_head.data(), (std::streamsize)outs->bam_head.size());
      }
      size_t total = 0, tooShort = 0, mapped = 0, notMapped = 0; IdSet seen;   // (id_set.hpp: a std::set of 10^6 IDs bounded the mapping phase)
      for (;;) {
        std::unique_ptr<Done> d = next(fi, seq);
        if (!d) break;
        if (d->file != fi) die("internal error: batch order");
        ++seq;
        for (size_t r = 0; r < d->names.size(); ++r) {
          ++total;
          const int len = d->lens[r], mlen = d->clens.empty() ? len : d->clens[r];   // (--hpc: the skips count compressed bases, the file carries raw lengths)
          if (mlen < w || mlen < k || mlen < minLen) { ++tooShort; continue; }
          // mapWrap.h:71-75 checks the IDs of mapping LINES against the reads already handled: a repeated ID only stops the run
          // when the repeat carries mappings; every handled read's ID is remembered (:154-157)
          if (d->off[r] == d->off[r + 1]) { ++notMapped; unm << len << "\t" << d->names[r] << "\n"; seen.insert(d->names[r]); continue; }
          if (!seen.insert(d->names[r])) die("Seems that read ID " + d->names[r] + " has already been processed");
          ++mapped;
        }
        if (compress) out.write(d->gz.data(), (std::streamsize)d->gz.size()); else out << d->text;
        for (size_t s = 0; s < N_SIDE; ++s) if (plan.side[s]) {
          sf[s].write(d->side[s].data(), (std::streamsize)d->side[s].size());
          std::string().swap(d->side[s]);
        }
        std::string().swap(d->gz);
        outs->append_sorted(fi, prefix, *d);
        if (keep_lines) { if (kept.size() <= fi) kept.resize(fi + 1); d->names.clear(); d->names.shrink_to_fit(); kept[fi].push_back(std::move(d)); }
      }
      if (keep_lines && kept.size() <= fi) kept.resize(fi + 1);
      if (compress) out.write((const char*)kBgzfEof, sizeof kBgzfEof);
      out.close();
      if (!out) die("Error writing " + out_name);
      for (size_t s = 0; s < N_SIDE; ++s) if (plan.side[s]) {
        if (kSideFiles[s].bgzf) sf[s].write((const char*)kBgzfEof, sizeof kBgzfEof);
        sf[s].close();
        if (!sf[s]) die("Error writing " + prefix + side_suffix((int)s, plan.reads.with_qual));
      }
      std::ofstream meta(prefix + ".meta");                      // mapWrap.h:178-184
      meta << "TotalReads " << total << "\nReadsTooShort " << tooShort << "\nReadsMapped " << mapped << "\nReadsNotMapped " << notMapped << "\n";
      std::ofstream ps(prefix + ".parameters");                  // mapWrap.h:196-211
      ps << "kmerSize " << k << "\nwindowSize " << w << "\nminReadLength " << minLen << "\nalphabetSize " << 4 << "\nreferenceSize " << refSize
         << "\npercentageIdentity " << pi << "\np_value " << pval << "\nrefSequences [" << ref << "]\nquerySequences [" << queries[fi]
         << "]\noutFileName " << prefix << "\nreportAll " << o.all << "\nindex " << "" << "\nmaximumMemory " << maxMem << "\n";
      if (hpc) ps << "hpc 1\n";
      std::cout << "INFO, [count of mapped reads, reads qualified for mapping, total input reads] = [" << mapped << ", " << total - tooShort << ", " << total << "]\n";
    }
  }

  void run_replicated() {
    // ---- workers: four contexts per device (--workers-per-gpu; three until round 4: with ten batches of 10^5 reads in one file the GPU idled
    // 60 % of the mapping phase), so that packing, result download and text formatting of one batch overlap the
    // kernels of the other; the device's chunk indexes are shared (read-only) by its contexts
    // The kernels of a batch fill the device; batches mapped side by side only take turns on it, and four workers that start together
    // then also finish together: they packed, fetched and formatted at the same time with the device idle, and mapped at the same time
    // in each other's way (the done-times of the workers came in groups of four, 60 ms apart).  So at most MAP_SLOTS batches per device are
    // inside their mapping section at a time (two: one fills the host-side gaps of the other), which staggers the workers.
    const size_t MAP_SLOTS = sw.map_slots;
    struct Slots {
      std::mutex m; std::condition_variable cv; size_t free_ = 0;
      void acquire() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return free_ > 0; }); --free_; }
      void release() { { std::lock_guard<std::mutex> lk(m); ++free_; } cv.notify_one(); }
    };
    std::vector<Slots> map_slots(G);
    for (auto& sl : map_slots) sl.free_ = MAP_SLOTS;
    std::vector<std::thread> workers;
    for (size_t d = 0; d < G; ++d) for (size_t wi = 0; wi < WPD; ++wi) workers.emplace_back([&, d, wi]() {
      mm_ctx* ctx = wi == 0 ? devs[d].ctx : wctx[d * WPD + wi];
      if (!ctx && mm_ctx_create(devs[d].phys, &ctx) != MM_OK) die("cannot create a worker context");
      while (std::unique_ptr<Batch> bt = reader.take()) {
        const auto t0 = std::chrono::steady_clock::now();
        ReadsPtr reads(upload_batch(ctx, *bt));
        std::vector<int> clens; if (hpc) clens = compressed_lengths(ctx, reads.get());
        const auto t1 = std::chrono::steady_clock::now();
        std::vector<mm_mapping*> parts;
        map_slots[d].acquire();
        const auto t1a = std::chrono::steady_clock::now();
        for (size_t c = 0; c < NC; ++c) parts.push_back(map_chunk(ctx, devs[d].idx[c], reads.get(), c ? parts[0] : nullptr));
        map_slots[d].release();
        mm_map_stats gst{}; if (sw.timing) mm_mapping_get_stats(parts[0], &gst);   // (device time of the batch's stages by the library's own events)
        mm_mapping* m = parts[0];
        if (parts.size() > 1) {                                   // unifyFiles: read-wise concatenation in chunk order
          ck(ctx, mm_mapping_concat(ctx, parts.data(), chunk_base.data(), (int)parts.size(), &m), "merge chunks");
          for (auto* pm : parts) mm_mapping_destroy(pm);
        }
        if (!plan.keep_reads()) reads.reset();                     // no side output needs them
        const auto t2 = std::chrono::steady_clock::now();
        const size_t seq = bt->seq;
        auto dn = finish_mapping(ctx, d, m, std::move(bt->names), std::move(bt->lens), std::move(clens), bt->file, std::move(reads));
        const auto t3 = std::chrono::steady_clock::now();
        auto secs = [](std::chrono::steady_clock::duration x) { return std::chrono::duration<double>(x).count(); };
        pc.add("5 reads pack+upload", secs(t1 - t0));
        pc.add("6 map", secs(t2 - t1a));
        pc.add("6a waited for the device", secs(t1a - t1));
        pc.add("7 mapq+fetch+format", secs(t3 - t2));
        if (sw.timing) {
          std::ostringstream os;
          os << "INFO, worker " << d << "." << wi << " batch " << seq << ": upload " << secs(t1 - t0) << " map " << secs(t2 - t1a)
             << " (waited " << secs(t1a - t1) << "; device ms: K1 " << gst.ms_minimizer << " K2 " << gst.ms_sketch << " K3 " << gst.ms_probe_gather
             << " K4 " << gst.ms_sort_hits + gst.ms_l1_scan << " K5 " << gst.ms_l2 << " all " << gst.ms_total << ") finish " << secs(t3 - t2)
             << " (mapq " << dn->t_mapq << " fetch " << dn->t_fetch << " format " << dn->t_format << ") done at +" << secs(t3 - pc.t0) << " s\n";
          std::cerr << os.str();
        }
        reader.recycle(std::move(bt));
        writer.put(seq, std::move(dn));
      }
      if (wi > 0) mm_ctx_destroy(ctx);
    });
    write_all([&](size_t fi, size_t seq) -> std::unique_ptr<Done> {
      std::unique_lock<std::mutex> lk(writer.m);
      for (;;) {
        { std::lock_guard<std::mutex> rl(reader.m); if (reader.file_end.size() > fi && reader.file_end[fi] == seq) return nullptr; }   // file fi ended before batch `seq`
        auto it = writer.ready.find(seq);
        if (it != writer.ready.end()) { auto d = std::move(it->second); writer.ready.erase(it); return d; }
        writer.cv.wait_for(lk, std::chrono::milliseconds(20));
      }
    });
    for (auto& t : workers) t.join();
  }

  void run_chunk_major() {
    // ---- sharded / streamed: every read batch is packed onto every device and stays there (2 bits per base) ...
    struct Held {
      size_t file = 0;
      std::vector<std::string> names;
      std::vector<int> lens, clens;                                // (clens: --hpc, the compressed lengths)
      std::vector<mm_seqset*> reads;                               // per device
      std::vector<mm_mapping*> sk;                                 // per device: the batch's minimizers + sketches (mm_sketch_batch), computed once for all chunks
      std::vector<mm_mapping*> part;                               // per chunk: the batch's records against that chunk, on the device that holds the chunk (c mod G)
      std::vector<std::vector<int64_t>> poff;                      // --host-gather: the same in host memory (rounds 1-3)
      std::vector<std::vector<mm_map_record>> prec;
    };
    // How the records of a batch reach the device that merges them (unifyFiles, mapWrap.h:128-145, in place of the PREFIX.N files):
    //   rccl  (several physical devices) mm_mapping_gather: ncclSend / ncclRecv over xGMI, one collective per batch
    //   peer  (logical devices of one GPU, or --peer-gather) mm_mapping_concat pulls the parts of other contexts with device-to-device copies
    //   host  (--host-gather) mm_mapping_fetch + mm_mapping_from_parts: through host memory, the path of rounds 1-3, kept as the cross-check
    bool distinct = true; for (size_t a = 0; a < G; ++a) for (size_t b2 = a + 1; b2 < G; ++b2) distinct = distinct && devs[a].phys != devs[b2].phys;
    enum class Gather { Rccl, Peer, Host };
    const Gather gather = o.v.count("host-gather") ? Gather::Host : (G > 1 && distinct && !o.v.count("peer-gather")) ? Gather::Rccl : Gather::Peer;
    if (sw.timing)
      std::cerr << "INFO, records of the chunks are gathered by "
                << (gather == Gather::Rccl ? "RCCL send / receive" : gather == Gather::Peer ? "device-to-device copies" : "the host") << "\n";
    std::vector<Held> held;
    while (std::unique_ptr<Batch> bt = reader.take()) {
      held.emplace_back();
      Held& h = held.back();
      h.file = bt->file; h.reads.assign(G, nullptr); h.sk.assign(G, nullptr); h.part.assign(NC, nullptr); h.poff.resize(NC); h.prec.resize(NC);
      on_each(G, [&](size_t d) { h.reads[d] = upload_batch(devs[d].ctx, *bt); });
      h.names = std::move(bt->names); h.lens = std::move(bt->lens);
      if (hpc) h.clens = compressed_lengths(devs[0].ctx, h.reads[0]);
      reader.recycle(std::move(bt));
    }
    pc.lap("5 reads pack+upload");
    // ... then the chunks in rounds: chunk c on device c mod N — all of them at once when they fit together (sharded), N at a time
    // otherwise (streamed: built, mapped, dropped).  A round's indexes are built concurrently, their thresholds follow in chunk
    // order from the accumulated histogram, then every device maps every batch against its chunks; the records of a pass go to the
    // host, where the reference keeps its PREFIX.N files (mapWrap.h:417-437).
    const size_t per_round = place == Place::Streamed ? G : NC;
    // Minimizers and sketches do not depend on the chunk: a batch keeps them on its device from its first chunk on (about 3 bytes per read
    // base, twelve times the packed reads), as long as all of them stay within an eighth of the device's memory; batches beyond that
    // recompute them per chunk (MM_CLI_NO_SKETCH_REUSE=1: all of them, the cross-check).
    std::vector<uint64_t> sk_used(G, 0), sk_budget(G, 0);
    for (size_t d = 0; d < G; ++d) {
      uint64_t tot = 0, fr = 0; char nm[8]; int cus = 0;
      if (mm_ctx_device_info(devs[d].ctx, nm, sizeof nm, &cus, &tot, &fr) == MM_OK && !sw.no_sketch_reuse) sk_budget[d] = tot / 8;
    }
    for (size_t c0 = 0; c0 < NC; c0 += per_round) {
      const size_t c1 = std::min(NC, c0 + per_round);
      on_each(G, [&](size_t d) { for (size_t c = c0; c < c1; ++c) if (c % G == d) build_chunk(devs[d], c); });
      for (size_t c = c0; c < c1; ++c) settle_threshold(c);
      pc.lap("3 index build");
      on_each(G, [&](size_t d) {
        for (size_t c = c0; c < c1; ++c) {
          if (c % G != d) continue;
          for (auto& h : held) {
            if (!h.sk[d] && sk_budget[d]) {
              uint64_t bases = 0; for (int L : (hpc ? h.clens : h.lens)) bases += (uint64_t)L;
              if (sk_used[d] + 3 * bases <= sk_budget[d]) { ck(devs[d].ctx, mm_sketch_batch(devs[d].ctx, h.reads[d], &mp, &h.sk[d]), "sketch"); sk_used[d] += 3 * bases; }
            }
            mm_mapping* pm = map_chunk(devs[d].ctx, devs[d].idx[c], h.reads[d], h.sk[d]);
            if (gather == Gather::Host) {
              h.poff[c].resize(h.names.size() + 1);
              ck(devs[d].ctx, mm_mapping_fetch(pm, h.poff[c].data(), nullptr, 0), "fetch");
              h.prec[c].resize((size_t)h.poff[c].back());
              ck(devs[d].ctx, mm_mapping_fetch(pm, h.poff[c].data(), h.prec[c].data(), (int64_t)h.prec[c].size()), "fetch");
              mm_mapping_destroy(pm);
            } else { ck(devs[d].ctx, mm_mapping_release_intermediates(pm), "release"); h.part[c] = pm; }   // the records stay where they were made
          }
          if (place == Place::Streamed) { mm_index_destroy(devs[d].idx[c]); devs[d].idx[c] = nullptr; }
        }
      });
      pc.lap("6 map");
    }
    // merge in chunk order (unifyFiles), mapping qualities over the union and text: batch b on device b mod N
    std::vector<std::unique_ptr<Done>> results(held.size());
    std::vector<int32_t> chunk_rank(NC); for (size_t c = 0; c < NC; ++c) chunk_rank[c] = (int32_t)(c % G);
    char comm_id[MM_COMM_ID_BYTES];
    if (gather == Gather::Rccl && mm_comm_unique_id(comm_id) != MM_OK) die("RCCL: cannot create a communicator id");
    std::vector<mm_mapping*> merged(held.size(), nullptr);
    on_each(G, [&](size_t d) {
      mm_ctx* ctx = devs[d].ctx;
      for (auto& h : held) { if (h.sk[d]) mm_mapping_destroy(h.sk[d]); mm_seqset_destroy(h.reads[d]); }
      if (gather == Gather::Rccl) {                                // every rank takes part in the gather of every batch, batch b ends on rank b mod G
        ck(ctx, mm_comm_init(ctx, comm_id, (int)d, (int)G), "RCCL communicator");
        for (size_t b = 0; b < held.size(); ++b) {
          Held& h = held[b];
          std::vector<mm_mapping*> mine; std::vector<int32_t> ids;
          for (size_t c = d; c < NC; c += G) { mine.push_back(h.part[c]); ids.push_back((int32_t)c); }
          mm_mapping* m = nullptr;
          ck(ctx, mm_mapping_gather(ctx, (int)(b % G), (int64_t)h.names.size(), (hpc ? h.clens : h.lens).data(), &mp, mine.data(), ids.data(), (int)mine.size(),
                                    (int)NC, chunk_rank.data(), chunk_base.data(), &m), "gather chunks");
          if (b % G == d) merged[b] = m;
          for (auto* pm : mine) mm_mapping_destroy(pm);
        }
        mm_comm_destroy(ctx);
      }
    });
    on_each(G, [&](size_t d) {
      for (size_t b = d; b < held.size(); b += G) {
        Held& h = held[b];
        mm_mapping* m = merged[b];
        if (gather == Gather::Peer) {
          ck(devs[d].ctx, mm_mapping_concat(devs[d].ctx, h.part.data(), chunk_base.data(), (int)NC, &m), "merge chunks");
        } else if (gather == Gather::Host) {
          std::vector<const int64_t*> op; std::vector<const mm_map_record*> rp;
          for (size_t c = 0; c < NC; ++c) { op.push_back(h.poff[c].data()); rp.push_back(h.prec[c].data()); }
          ck(devs[d].ctx, mm_mapping_from_parts(devs[d].ctx, (int64_t)h.names.size(), (hpc ? h.clens : h.lens).data(), &mp, (int)NC, op.data(), rp.data(), chunk_base.data(), &m), "merge chunks");
        }
        results[b] = finish_mapping(devs[d].ctx, d, m, std::move(h.names), std::move(h.lens), std::move(h.clens), h.file);
        std::vector<std::vector<int64_t>>().swap(h.poff); std::vector<std::vector<mm_map_record>>().swap(h.prec);
      }
    });
    if (gather == Gather::Peer) for (auto& h : held) for (size_t c = 0; c < NC; ++c) if (h.part[c]) {   // (after every owner has pulled what it needed; destroyed through its own context)
      mm_mapping_destroy(h.part[c]); h.part[c] = nullptr; }
    pc.lap("7 mapq+fetch+format");
    write_all([&](size_t fi, size_t seq) -> std::unique_ptr<Done> {
      if (seq >= results.size() || results[seq]->file != fi) return nullptr;
      return std::move(results[seq]);
    });
  }

  // --then-classify DBDIR (not in the reference): `metamaps classify --DB DBDIR --mappings PREFIX` for every output prefix, in THIS process, on the
  // files just written — the same code (classify_one) on the same bytes, so the same .EM* files as the two-process form, which stays the tested
  // default.  What it saves is what lies between the two processes: this one's exit (150 GB of index handed back), the next one's HIP
  // initialisation behind it (1.3-1.9 s waiting for the driver) and its contexts: the live contexts are used.
  void then_classify() {
    if (!o.v.count("then-classify") || only_index) return;
    if (reader.th.joinable()) reader.th.join();
    const EmReduce reduce = o.em_host ? EmReduce::Host : ((devs.size() > 1 || o.v.count("gpus") || o.v.count("devices")) ? EmReduce::Rccl : EmReduce::None);
    const ClassifyOpts copts = classify_options(o, mode);         // (main has refused what is malformed)
    // the last prefix ends the process from inside classify_one, as the last file of `classify` does: everything is written and closed, the
    // gigabyte of line tables and text is not taken apart first (MM_CLI_FULL_TEARDOWN=1: the orderly way)
    const std::function<void()> leave = [&] { pc.lap("9 classify"); pc.report(); };
    for (size_t fi = 0; fi < prefixes.size(); ++fi) {
      const bool last = fi + 1 == prefixes.size();
      KeptLines kl; kl.cname = &cname;
      if (keep_lines && fi < kept.size())
        for (const auto& d : kept[fi]) kl.parts.push_back(KeptLines::Part{d->text.data(), d->meta.data(), d->meta.size(), d->off.data(), d->lens.size()});
      classify_one(devs, reduce, prefixes[fi], o.v.at("then-classify"), copts, ClassifyHooks{last ? leave : std::function<void()>(), nullptr}, keep_lines ? &kl : nullptr, sw);
      if (keep_lines && fi < kept.size()) kept[fi].clear();
      for (auto& d : devs) mm_comm_destroy(d.ctx);
      pc.lap("9 classify");
    }
  }

  int run() {
    read_parameters();
    outs.emplace(plan, sw, prefixes.size());
    open_devices();
    if (!from_index) {
      load_reference();
      plan_chunks();
      if (only_index) return write_index_files();
    } else read_index_files(ipre, cname, clen, ref_bases, chunks);   // `metamaps mapAgainstIndex` (mapWrap.h:443-554)
    decide_placement();
    build_resident_indexes();
    mp = mm_map_params{k, w, pi, minLen};
    for (auto& ch : chunks) chunk_base.push_back(ch.first);
    outs->deflate_bam_header(ctx0, cname, clen);                 // (before the workers take the first device's context)
    start_reader();
    if (prewarm.joinable()) prewarm.join();
    if (place != Place::Replicated) for (auto*& c : wctx) if (c) { mm_ctx_destroy(c); c = nullptr; }   // (the other modes drive one context per device)
    if (place == Place::Replicated) run_replicated(); else run_chunk_major();
    pc.lap("8 write");
    outs->write(ctx0, refset[0], prefixes, cname, clen);
    then_classify();
    if (!sw.full_teardown) { if (reader.th.joinable()) reader.th.join(); pc.report(); finish_fast(); }
    drop_refsets();
    for (auto& d : devs) { for (auto* ix : d.idx) if (ix) mm_index_destroy(ix); mm_ctx_destroy(d.ctx); }
    return 0;
  }
};

int map_mode(const Options& o, const std::string& mode, const CliSwitches& sw, const OutputPlan& plan) { MapRun run(o, mode, sw, plan); return run.run(); }

}  // namespace
